#!/usr/bin/env python3
"""What an occupancy grid buys on a trained scene: trains the sphere scene of tools/train_demo.py (1500 steps), fills a 128^3
grid from both models, and renders a 400 x 400, 64 + 128 view culled and un-culled, alternating, after warm-up; device events
around each view (a view ends in a synchronise).  Writes profiles/occupancy_render.json: fill time, occupied fraction, live
fractions per pass, both view times with their spread, the overhead of an all-live grid, PSNR of the culled render against the
un-culled one and of each against the analytic ground truth.

    python tools/occupancy_bench.py [--steps 1500] [--reps 9] [--bench-json FILE] [--out profiles/occupancy_render.json]

--bench-json: a file holding bench.py's result line from the same machine; its rate is recorded beside the un-culled leg
(the same 400 x 400, 64 + 128 workload on random weights), which is the baseline the culled time is reported against.
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

BOX = [[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]]          # the unit sphere with room for the dilation


def timed(fn):
    """Milliseconds of device time of fn() between two events; fn's work is complete when this returns."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def psnr(a, b):
    return float(utils.mse2psnr(utils.img2mse(a, b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--bench-json", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy_render.json"))
    a = ap.parse_args()

    train, (coarse, fine, _, _, _, _, poses_t, _, i_test) = train_demo.run(steps=a.steps, verbose=False)
    dev = torch.device("cuda:0")
    H = W = a.res
    K = synth.lego_intrinsics(H, W)
    pose = poses_t[i_test, :3, :4]
    r = render_utils.Renderer(perturb=0.0, N_importance=128, N_samples=64, use_viewdirs=True, white_bkgd=True, raw_noise_std=0.0,
                              near=2.0, far=6.0)

    grid = occupancy.OccupancyGrid(BOX, a.grid, outside="empty", device=dev)
    fill_ms, _ = timed(lambda: grid.fill_from_density([coarse, fine]))
    all_live = occupancy.OccupancyGrid(BOX, a.grid, outside="live", device=dev)

    def view(g):
        r.occupancy = g
        with torch.no_grad():
            return r.render(H, W, K, coarse, fine, chunk=32768, c2w=pose, retraw=False)[0]

    legs = {"unculled": None, "culled": grid, "all_live": all_live}
    times = {k: [] for k in legs}
    images, cull = {}, {}
    for i in range(a.warmup + a.reps):
        for name, g in legs.items():             # alternating: every leg sees the same clocks and the same neighbours
            ms, img = timed(lambda: view(g))
            if i >= a.warmup:
                times[name].append(ms)
            images[name] = img
            if g is not None:
                cull[name] = dict(r.last_cull)
    r.occupancy = None
    truth = train_demo.sphere_image(H, W, K, pose.cpu().numpy(), dev).to(dev)
    c = cull["culled"]
    out = {
        "workload": "sphere scene of tools/train_demo.py, %d steps; %dx%d view, 64 + 128 samples, perturb 0, chunk 32768" % (a.steps, H, W),
        "train": train,
        "grid": {"resolution": a.grid, "box": BOX, "outside": "empty", "samples_per_cell": 4, "dilate": 1, "fill_ms": fill_ms,
                 "occupied_fraction": grid.occupied_fraction()},
        "live_fraction": {"coarse": c["coarse_live"] / c["coarse_total"], "fine": c["fine_live"] / c["fine_total"], "counts": c},
        "view_ms": {k: spread(v) for k, v in times.items()},
        "culled_over_unculled": statistics.median(times["culled"]) / statistics.median(times["unculled"]),
        "all_live_over_unculled": statistics.median(times["all_live"]) / statistics.median(times["unculled"]),
        "unculled_rays_per_s": H * W / (statistics.median(times["unculled"]) * 1e-3),
        "psnr": {"culled_vs_unculled": psnr(images["culled"], images["unculled"]),
                 "all_live_equals_unculled": bool(torch.equal(images["all_live"], images["unculled"])),
                 "unculled_vs_truth": psnr(images["unculled"], truth), "culled_vs_truth": psnr(images["culled"], truth)},
    }
    if a.bench_json and os.path.exists(a.bench_json):
        with open(a.bench_json) as f:
            lines = [ln for ln in f.read().splitlines() if ln.startswith("{")]
        if lines:
            b = json.loads(lines[-1])
            out["bench_py_same_machine"] = {"rays_per_s": b.get("value"), "ms_per_step": b.get("ms_per_step"),
                                            "perturb0_ms_per_step": (b.get("perturb0") or {}).get("ms_per_step")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
