#!/usr/bin/env python3
"""What the ray bounds (occupancy.RayBounds, Renderer.ray_bounds) buy on a trained scene, in the set-up of
tools/occupancy_bench.py: the sphere scene of tools/train_demo.py after 1500 steps, a 128^3 grid over [-1.5, 1.5]^3 filled from
both models, outside = 'empty', a 400 x 400 view, perturb 0, bf16.  Four legs alternate in one process (median of 9 after 2
warm-ups, min - max recorded):

    culled            occupancy grid, no bounds, 64 + 128     (the leg of profiles/occupancy_render.json)
    culled_bounds     occupancy grid + bounds, 64 + 128
    culled_bounds_half  occupancy grid + bounds, 32 + 64
    unculled_bounds   bounds alone, 64 + 128

Per leg: ms per view, PSNR against the analytic ground truth and against the first leg.  Once: the device time of the bounds
kernel alone on the view's 160 000 rays, the share of rays hit, the mean (far' - near') / (far - near), and -- information
only -- the share of the un-clipped render's live samples (coarse ladder and fine z_vals) that fall outside the bounds.
A second table trains with the bounds on (train_demo.run(..., ray_bounds_probes=P, ray_bounds_pad=1 / 8 / 32)) and records the
test PSNR at 64 + 128 and at 32 + 64 against the dense-trained run of the same seed -- rendered with the run's own bounds, with
none, with bounds and cull, with the cull alone -- and the same for the culled run trained without bounds, rendered with bounds.  Writes profiles/occupancy_bounds.json.

    python tools/occupancy_bounds_bench.py [--steps 1500] [--reps 9] [--probes 256] [--pad 1]
                                           [--bench-this A.json B.json C.json --bench-parent A.json B.json C.json]

--bench-this / --bench-parent: files holding bench.py's result line, of this tree and of the parent commit's build, run
alternating on the same machine; the six values are recorded with the verdict "unchanged" = this tree's three values lie
within the range of the parent's three, widened by the parent's own spread (max - min).
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


def bench_values(files):
    vals = []
    for path in files or []:
        with open(path) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        b = json.loads(lines[-1])
        vals.append({"rays_per_s": b.get("value"), "ms_per_step": b.get("ms_per_step")})
    return vals


def outside_share(r, grid, batch, bounds, coarse, fine, chunk=32768):
    """Of the samples of the un-clipped, un-culled render that look up live -- the coarse ladder and the fine pass's z_vals --
    the share that lies outside [near', far'].  Information only."""
    live = out = 0
    with torch.no_grad():
        for i in range(0, batch.shape[0], chunk):
            rays, b = batch[i:i + chunk], bounds[i:i + chunk]
            z_f = r.render_rays(rays, coarse, fine, retweights=True)["z_vals"]
            t = torch.linspace(0., 1., int(r.N_samples), device=rays.device)
            z_c = rays[:, 6:7] * (1. - t) + rays[:, 7:8] * t
            for z in (z_c, z_f):
                on = grid.query(rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None])
                live += int(on.sum())
                out += int((on & ((z < b[:, :1]) | (z > b[:, 1:]))).sum())
    return {"live_samples": live, "outside_bounds": out, "share": out / max(live, 1)}


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
    ap.add_argument("--train-pads", type=int, nargs="*", default=[1, 8, 32], help="ray_bounds_pad of the runs of the second table")
    ap.add_argument("--bench-this", nargs="*", default=None)
    ap.add_argument("--bench-parent", nargs="*", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy_bounds.json"))
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

    def view(g, bounds, nc, ni):
        r.occupancy, r.ray_bounds, r.N_samples, r.N_importance = g, bounds, nc, ni
        with torch.no_grad():
            return r.render(H, W, K, coarse, fine, chunk=32768, c2w=pose, retraw=False)[0]

    legs = {"culled": (grid, None, 64, 128), "culled_bounds": (grid, rb, 64, 128), "culled_bounds_half": (grid, rb, 32, 64),
            "unculled_bounds": (None, rb, 64, 128)}
    times = {k: [] for k in legs}
    images, cull = {}, {}
    for i in range(a.warmup + a.reps):
        for name, leg in legs.items():           # alternating: every leg sees the same clocks and the same neighbours
            ms, img = timed(lambda: view(*leg))
            if i >= a.warmup:
                times[name].append(ms)
            images[name] = img
            if leg[0] is not None:
                cull[name] = dict(r.last_cull)
    r.occupancy, r.ray_bounds, r.N_samples, r.N_importance = None, None, 64, 128
    truth = train_demo.sphere_image(H, W, K, pose.cpu().numpy(), dev).to(dev)

    # the bounds kernel alone, on the view's rays
    batch = utils.make_ray_batch(H, W, K, pose, r.near, r.far, True, False, device=dev)
    kernel_ms = []
    for i in range(a.warmup + a.reps):
        ms, clipped = timed(lambda: rb.apply(batch))
        if i >= a.warmup:
            kernel_ms.append(ms)
    bounds, span = grid.ray_bounds(batch, a.probes, a.pad)
    hit = span[:, 0] >= 0
    ratio = (bounds[:, 1] - bounds[:, 0]) / (batch[:, 7] - batch[:, 6])
    out = {
        "workload": "sphere scene of tools/train_demo.py, %d steps; %dx%d view, perturb 0, bf16, chunk 32768; legs alternating, "
                    "median of %d after %d warm-ups" % (a.steps, H, W, a.reps, a.warmup),
        "train": train,
        "grid": {"resolution": a.grid, "box": BOX, "outside": "empty", "occupied_fraction": grid.occupied_fraction()},
        "ray_bounds": {"probes": a.probes, "pad": a.pad, "kernel_ms": spread(kernel_ms), "rays": int(batch.shape[0]),
                       "rays_hit_share": float(hit.float().mean()), "mean_span_ratio_all_rays": float(ratio.mean()),
                       "mean_span_ratio_hit_rays": float(ratio[hit].mean()) if bool(hit.any()) else None,
                       "live_dense_samples_outside_bounds": outside_share(r, grid, batch, bounds, coarse, fine)},
        "legs": {name: {"samples": "%d + %d" % (leg[2], leg[3]), "occupancy": leg[0] is not None, "bounds": leg[1] is not None,
                        "view_ms": spread(times[name]), "psnr_vs_truth": psnr(images[name], truth),
                        "psnr_vs_culled": None if name == "culled" else psnr(images[name], images["culled"]),
                        "over_culled": statistics.median(times[name]) / statistics.median(times["culled"]),
                        "live_counts": cull.get(name)} for name, leg in legs.items()},
    }

    # models trained with the bounds on, against the dense-trained run of the same seed
    def test_psnr(state, nc, ni):
        c, f, _, _, rend, (h, w, k), poses, imgs, it = state
        keep = rend.N_samples, rend.N_importance, rend.perturb
        rend.N_samples, rend.N_importance, rend.perturb = nc, ni, 0.0
        with torch.no_grad():
            rgb = rend.render(h, w, k, c, f, chunk=32768, c2w=poses[it, :3, :4], retraw=False)[0]
        rend.N_samples, rend.N_importance, rend.perturb = keep
        return psnr(rgb, imgs[it])

    def evals(state, rb, occ=None):
        rend = state[4]
        keep = rend.ray_bounds, rend.occupancy
        rend.ray_bounds, rend.occupancy = rb, occ
        res = {"psnr_64_128": test_psnr(state, 64, 128), "psnr_32_64": test_psnr(state, 32, 64)}
        rend.ray_bounds, rend.occupancy = keep
        return res

    def run_of(**kw):
        return train_demo.run(steps=a.train_steps, seed=0, verbose=False, **kw)

    dense_out, dense_state = run_of()
    table = {"run": "train_demo.run(steps=%d, seed=0, occupancy_res=32, occupancy_warmup=200, occupancy_refresh=16, ray_bounds_probes=%d, "
                    "ray_bounds_pad=PAD); psnr_after: the run's own figure (test view, the training perturb, its own bounds); every "
                    "other figure: the same test view at perturb 0, at 64 + 128 and at 32 + 64 samples, rendered with the run's own "
                    "bounds, with no bounds, with its bounds and its grid as Renderer.occupancy, and with that cull alone"
                    % (a.train_steps, a.probes),
             "dense": dict(psnr_after=dense_out["psnr_after"], steps_per_s=dense_out["steps_per_s"], no_bounds=evals(dense_state, None))}
    for pad in a.train_pads:
        clip_out, clip_state = run_of(occupancy_res=32, occupancy_warmup=200, occupancy_refresh=16, ray_bounds_probes=a.probes,
                                      ray_bounds_pad=pad)
        own = clip_state[4].ray_bounds
        table["pad_%d" % pad] = {"psnr_after": clip_out["psnr_after"], "steps_per_s": clip_out["steps_per_s"],
                                 "stats": clip_out["occupancy"]["stats"], "own_bounds": evals(clip_state, own),
                                 "no_bounds": evals(clip_state, None), "own_bounds_and_cull": evals(clip_state, own, own.grid),
                                 "cull_only": evals(clip_state, None, own.grid)}
    # the culled run without bounds (tools/occupancy_train_bench.py's learning run), rendered with bounds at inference only
    cull_out, cull_state = run_of(occupancy_res=32, occupancy_warmup=200, occupancy_refresh=16)
    g32 = occupancy.OccupancyGrid(train_demo.SPHERE_BOX, 32, outside="empty", device=dev).fill_from_density([cull_state[0], cull_state[1]])
    table["culled_without_bounds"] = {"psnr_after": cull_out["psnr_after"], "stats": cull_out["occupancy"]["stats"],
                                      "no_bounds": evals(cull_state, None),
                                      "bounds_pad_1": evals(cull_state, occupancy.RayBounds(g32, a.probes, 1)),
                                      "bounds_pad_8": evals(cull_state, occupancy.RayBounds(g32, a.probes, 8)),
                                      "cull_only": evals(cull_state, None, g32)}
    out["trained_with_bounds"] = table

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
