#!/usr/bin/env python3
"""What the live-stretch coarse sampler (occupancy.LiveSampler, Renderer.coarse_sampler) buys on a trained scene, by the
protocol of tools/occupancy_bounds_bench.py: the sphere scene of tools/train_demo.py after 1500 steps, a 128^3 grid over
[-1.5, 1.5]^3 filled from both models, outside = 'empty', a 400 x 400 view, perturb 0, bf16.  Five legs alternate in one process
(median of 9 after 2 warm-ups, min - max recorded):

    culled                 occupancy grid, 64 + 128              (the leg of profiles/occupancy_render.json)
    culled_bounds          occupancy grid + ray bounds, 64 + 128 (the leg of profiles/occupancy_bounds.json)
    culled_sampler         occupancy grid + sampler, 64 + 128
    culled_sampler_32_64   occupancy grid + sampler, 32 + 64
    culled_sampler_16_32   occupancy grid + sampler, 16 + 32

Per leg: ms per view, PSNR against the analytic ground truth and against the first leg, the live coarse and fine points, and
the share of the coarse samples of the rays that hit the grid (a live probe) which look up live.  Once: the device time of the
sampler's kernel alone on the view's 160 000 rays at 64, 32 and 16 samples, beside nerf_amd_coarse_z's at 64.
A second table trains with the sampler on (train_demo.run(steps=600, seed=0, occupancy_res=32, live_sampler_probes=P,
live_sampler_pad=1 / 8 / 32)) against the dense run and the culled run of the same seed; the dense run's spread over three
seeds (profiles/occupancy_train.json) is the margin to read it by.  Writes profiles/occupancy_sampler.json.

    python tools/occupancy_sampler_bench.py [--steps 1500] [--reps 9] [--probes 256] [--pad 1]
                                            [--bench-this A.json B.json C.json --bench-parent A.json B.json C.json]

--bench-this / --bench-parent: as in tools/occupancy_bounds_bench.py (bench.py's result lines of this tree and of the parent
commit's build, run alternating on the same machine).
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
import torch  # noqa: E402

import train_demo  # noqa: E402
from nerf_shared_amd import occupancy, render_utils, synth, utils  # noqa: E402
from occupancy_bench import BOX, psnr, spread, timed  # noqa: E402
from occupancy_bounds_bench import bench_values  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--probes", type=int, default=256)
    ap.add_argument("--pad", type=int, default=1)
    ap.add_argument("--train-steps", type=int, default=600, help="steps of the runs of the second table")
    ap.add_argument("--train-pads", type=int, nargs="*", default=[1, 8, 32], help="live_sampler_pad of the runs of the second table")
    ap.add_argument("--bench-this", nargs="*", default=None)
    ap.add_argument("--bench-parent", nargs="*", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy_sampler.json"))
    a = ap.parse_args()

    train, (coarse, fine, _, _, _, _, poses_t, _, i_test) = train_demo.run(steps=a.steps, verbose=False)
    dev = torch.device("cuda:0")
    H = W = a.res
    K = synth.lego_intrinsics(H, W)
    pose = poses_t[i_test, :3, :4]
    r = render_utils.Renderer(perturb=0.0, N_importance=128, N_samples=64, use_viewdirs=True, white_bkgd=True, raw_noise_std=0.0,
                              near=2.0, far=6.0)
    grid = occupancy.OccupancyGrid(BOX, a.grid, outside="empty", device=dev)
    grid.fill_from_density([coarse, fine])
    rb = occupancy.RayBounds(grid, a.probes, a.pad)
    ls = occupancy.LiveSampler(grid, a.probes, a.pad)

    def view(bounds, sampler, nc, ni):
        r.occupancy, r.ray_bounds, r.coarse_sampler, r.N_samples, r.N_importance = grid, bounds, sampler, nc, ni
        with torch.no_grad():
            return r.render(H, W, K, coarse, fine, chunk=32768, c2w=pose, retraw=False)[0]

    legs = {"culled": (None, None, 64, 128), "culled_bounds": (rb, None, 64, 128), "culled_sampler": (None, ls, 64, 128),
            "culled_sampler_32_64": (None, ls, 32, 64), "culled_sampler_16_32": (None, ls, 16, 32)}
    times = {k: [] for k in legs}
    images, cull = {}, {}
    for i in range(a.warmup + a.reps):
        for name, leg in legs.items():           # alternating: every leg sees the same clocks and the same neighbours
            ms, img = timed(lambda: view(*leg))
            if i >= a.warmup:
                times[name].append(ms)
            images[name] = img
            cull[name] = dict(r.last_cull)
    r.occupancy, r.ray_bounds, r.coarse_sampler, r.N_samples, r.N_importance = None, None, None, 64, 128
    truth = train_demo.sphere_image(H, W, K, pose.cpu().numpy(), dev).to(dev)

    # where each leg's coarse samples are: of the rays with a live probe, the share of coarse samples that look up live
    batch = utils.make_ray_batch(H, W, K, pose, r.near, r.far, True, False, device=dev)
    hit = grid.coarse_depths(batch, torch.linspace(0., 1., 2, device=dev), a.probes, a.pad)[1] > 0

    def coarse_live_share(bounds, sampler, nc):
        rays = batch if bounds is None else bounds.apply(batch)
        t = torch.linspace(0., 1., nc, device=dev)
        z = rays[:, 6:7] * (1. - t) + rays[:, 7:8] * t if sampler is None else grid.coarse_depths(rays, t, sampler.probes, sampler.pad)[0]
        on = torch.cat([grid.query(rays[i:i + 32768, None, 0:3] + rays[i:i + 32768, None, 3:6] * z[i:i + 32768, :, None])
                        for i in range(0, rays.shape[0], 32768)], 0)
        return float(on[hit].float().mean())

    # the kernel alone, on the view's rays
    def kernel_ms(fn):
        ms = []
        for i in range(a.warmup + a.reps):
            t, _ = timed(fn)
            if i >= a.warmup:
                ms.append(t)
        return spread(ms)

    kernel = {}
    for nc in (64, 32, 16):
        r.N_samples = nc
        z = torch.empty(batch.shape[0], nc, device=dev)
        r.coarse_sampler = ls
        kernel["sampler_%d" % nc] = kernel_ms(lambda: r._coarse_z(batch, None, z))
        r.coarse_sampler = None
        if nc == 64:
            kernel["nerf_amd_coarse_z_64"] = kernel_ms(lambda: r._coarse_z(batch, None, z))
    r.N_samples = 64

    out = {
        "workload": "sphere scene of tools/train_demo.py, %d steps; %dx%d view, perturb 0, bf16, chunk 32768; legs alternating, "
                    "median of %d after %d warm-ups" % (a.steps, H, W, a.reps, a.warmup),
        "train": train,
        "grid": {"resolution": a.grid, "box": BOX, "outside": "empty", "occupied_fraction": grid.occupied_fraction()},
        "sampler": {"probes": a.probes, "pad": a.pad, "rays": int(batch.shape[0]), "rays_hit_share": float(hit.float().mean()),
                    "kernel_ms": kernel},
        "legs": {name: {"samples": "%d + %d" % (leg[2], leg[3]), "bounds": leg[0] is not None, "sampler": leg[1] is not None,
                        "view_ms": spread(times[name]), "psnr_vs_truth": psnr(images[name], truth),
                        "psnr_vs_culled": None if name == "culled" else psnr(images[name], images["culled"]),
                        "over_culled": statistics.median(times[name]) / statistics.median(times["culled"]),
                        "live_counts": cull[name], "coarse_live_share_of_hit_rays": coarse_live_share(leg[0], leg[1], leg[2])}
                 for name, leg in legs.items()},
    }

    # models trained with the sampler on, against the dense and the culled run of the same seed
    def test_psnr(state, nc, ni):
        c, f, _, _, rend, (h, w, k), poses, imgs, it = state
        keep = rend.N_samples, rend.N_importance, rend.perturb
        rend.N_samples, rend.N_importance, rend.perturb = nc, ni, 0.0
        with torch.no_grad():
            rgb = rend.render(h, w, k, c, f, chunk=32768, c2w=poses[it, :3, :4], retraw=False)[0]
        rend.N_samples, rend.N_importance, rend.perturb = keep
        return psnr(rgb, imgs[it])

    def evals(state, sampler):
        rend = state[4]
        keep = rend.coarse_sampler
        rend.coarse_sampler = sampler
        res = {"psnr_64_128": test_psnr(state, 64, 128), "psnr_32_64": test_psnr(state, 32, 64)}
        rend.coarse_sampler = keep
        return res

    def run_of(**kw):
        return train_demo.run(steps=a.train_steps, seed=0, verbose=False, **kw)

    with open(os.path.join(REPO, "profiles", "occupancy_train.json")) as f:
        margin = float(json.load(f)["learning"]["dense_psnr_spread"])
    dense_out, dense_state = run_of()
    cull_out, cull_state = run_of(occupancy_res=32, occupancy_warmup=200, occupancy_refresh=16)
    table = {"run": "train_demo.run(steps=%d, seed=0, occupancy_res=32, occupancy_warmup=200, occupancy_refresh=16, live_sampler_probes=%d, "
                    "live_sampler_pad=PAD); psnr_after: the run's own figure (test view, the training perturb, its own sampler); "
                    "own_sampler / no_sampler: the same test view at perturb 0, at 64 + 128 and at 32 + 64 samples" % (a.train_steps, a.probes),
             "dense_psnr_spread_over_three_seeds": margin,
             "dense": dict(psnr_after=dense_out["psnr_after"], steps_per_s=dense_out["steps_per_s"], no_sampler=evals(dense_state, None)),
             "culled": dict(psnr_after=cull_out["psnr_after"], steps_per_s=cull_out["steps_per_s"], stats=cull_out["occupancy"]["stats"],
                            no_sampler=evals(cull_state, None))}
    for pad in a.train_pads:
        s_out, s_state = run_of(occupancy_res=32, occupancy_warmup=200, occupancy_refresh=16, live_sampler_probes=a.probes,
                                live_sampler_pad=pad)
        own = s_state[4].coarse_sampler
        table["pad_%d" % pad] = {"psnr_after": s_out["psnr_after"], "steps_per_s": s_out["steps_per_s"],
                                 "below_dense_db": dense_out["psnr_after"] - s_out["psnr_after"],
                                 "within_margin": s_out["psnr_after"] >= dense_out["psnr_after"] - margin,
                                 "stats": s_out["occupancy"]["stats"], "own_sampler": evals(s_state, own), "no_sampler": evals(s_state, None)}
    out["trained_with_sampler"] = table

    this, parent = bench_values(a.bench_this), bench_values(a.bench_parent)
    if this and parent:
        pv, tv = [b["ms_per_step"] for b in parent], [b["ms_per_step"] for b in this]
        sp = max(pv) - min(pv)
        out["bench_py_default_path"] = {"parent_ms_per_step": pv, "this_ms_per_step": tv, "parent": parent, "this": this,
                                        "parent_spread_ms": sp, "accepted_range_ms": [min(pv) - sp, max(pv) + sp],
                                        "unchanged": all(min(pv) - sp <= v <= max(pv) + sp for v in tv)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
