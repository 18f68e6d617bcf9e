#!/usr/bin/env python
"""What leaving out the colour branch of empty sample blocks buys (nerf_amd_set_tuning key 3; csrc/mlp_bf16_s16.hip
view_branch_fold), scene by scene: a 400x400 view, 64 + 128 samples, perturb 0, bf16, chunk 32768, rendered with the skip on
(key 3 = 0) and off (key 3 = 1) alternately in one process -- median / min / max of --reps views after --warmup -- for
  sphere   the trained sphere of tools/train_demo.py (a scene with content and empty space around it)
  mixed    random weights sharpened x3, seeds 1 / 19 (sigma changes sign along every ray)
  dense    the same with alpha_linear.bias = +1e3: nothing can be skipped -- what the decision itself costs
  empty    the same with alpha_linear.bias = -1e3: everything is skipped -- the upper bound, like bench.py's view
and the share of 16-point blocks (and of 32-point waves with one / both blocks empty) per pass, counted on the host from the
sigma of the off leg's raw, launch group by launch group.  The maps of both legs are compared on raw bits."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import torch  # noqa: E402

from nerf_shared_amd import _lib, nerf, render_utils, synth, utils  # noqa: E402

ARCH = dict(D=8, W=256, output_ch=5, skips=[4], use_viewdirs=True, multires=10, multires_views=4)
GROUP = 32768
CFG = dict(perturb=0.0, N_importance=128, N_samples=64, use_viewdirs=True, white_bkgd=True, raw_noise_std=0.0, near=2.0, far=6.0)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def synthetic(dev, seed, alpha_bias):
    sd = synth.torch_state_dict(seed, 3.0, **{**ARCH, "skips": (4,)})
    if alpha_bias is not None:
        sd["alpha_linear.bias"].fill_(alpha_bias)
    m = nerf.NeRF(**ARCH)
    m.load_state_dict(sd)
    m.precision = "bf16"
    return m.to(dev).requires_grad_(False)


def block_shares(raw):
    """raw [R, S, 4] of one launch: (blocks, empty blocks, waves, waves with one block empty, waves with both)."""
    sigma = raw[..., 3].reshape(-1)
    n = sigma.numel()
    dead = torch.cat([sigma <= 0, torch.ones(-n % 32, dtype=torch.bool, device=raw.device)]).view(-1, 2, 16).all(2)
    per_wave = dead.sum(1)
    n_blocks = -(-n // 16)
    return n_blocks, int(dead.sum()) - (dead.numel() - n_blocks), dead.shape[0], int((per_wave == 1).sum()), int((per_wave == 2).sum())


def count_blocks(r, batch, coarse, fine):
    """Per pass, summed over the launch groups of the view, with the skip off (raw to the caller switches it off anyway)."""
    r0 = render_utils.Renderer(**dict(CFG, N_importance=0))
    tot = {"coarse": [0] * 5, "fine": [0] * 5}
    with torch.no_grad():
        for i in range(0, batch.shape[0], GROUP):
            rows = batch[i:i + GROUP]
            for name, raw in (("coarse", r0.render_rays(rows, coarse, None, retraw=True)["raw"]),
                              ("fine", r.render_rays(rows, coarse, fine, retraw=True)["raw"])):
                tot[name] = [x + y for x, y in zip(tot[name], block_shares(raw))]
    out = {}
    for name, (nb, eb, nw, w1, w2) in tot.items():
        out[name] = {"blocks": nb, "empty_blocks": eb, "share_of_blocks_skipped": eb / nb, "waves": nw,
                     "share_of_waves_all_skipped": w2 / nw, "share_of_waves_half_skipped": w1 / nw}
    mf = (out["coarse"]["empty_blocks"] + out["fine"]["empty_blocks"]) / (out["coarse"]["blocks"] + out["fine"]["blocks"])
    out["share_of_all_blocks_skipped"] = mf
    out["share_of_mfmas_skipped"] = mf * 152 / 2088
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train-steps", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--res", type=int, default=400)
    ap.add_argument("--scenes", default="sphere,mixed,dense,empty")
    ap.add_argument("--out", default=os.path.join(REPO, "logs", "view_skip_scenes.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = a.res
    K = synth.lego_intrinsics(H, W)
    r = render_utils.Renderer(**CFG)
    result = {"protocol": "one process, key 3 = 0 (skip) and 1 (never) alternating view by view, %d views each after %d warm-ups; device "
                          "time of Renderer.render(%d, %d, chunk=32768, perturb 0, bf16) between two events" % (a.reps, a.warmup, H, W),
              "scenes": {}}
    for scene in a.scenes.split(","):
        if scene == "sphere":
            import train_demo
            _, (coarse, fine, _, _, _, _, poses_t, _, i_test) = train_demo.run(steps=a.train_steps, verbose=False)
            pose = poses_t[i_test, :3, :4]
            coarse.precision = fine.precision = "bf16"
        else:
            bias = {"mixed": None, "dense": 1e3, "empty": -1e3}[scene]
            coarse, fine = synthetic(dev, 1, bias), synthetic(dev, 19, bias)
            pose = torch.tensor(synth.LEGO_C2W, dtype=torch.float32, device=dev)[:3, :4]

        def view():
            with torch.no_grad():
                return r.render(H, W, K, coarse, fine, chunk=GROUP, c2w=pose, retraw=False)

        times, maps = {"skip": [], "never": []}, {}
        for i in range(a.warmup + a.reps):
            for leg, value in (("skip", 0), ("never", 1)):
                _lib.check(_lib.lib.nerf_amd_set_tuning(3, value), "set_tuning")
                ms, out = timed(view)
                if i >= a.warmup:
                    times[leg].append(ms)
                maps[leg] = [t.clone() for t in out[:3]]
        _lib.lib.nerf_amd_set_tuning(3, 0)
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(maps["skip"], maps["never"]))
        batch = utils.make_ray_batch(H, W, K, pose, CFG["near"], CFG["far"], True, False, device=dev)
        s, n = spread(times["skip"]), spread(times["never"])
        result["scenes"][scene] = {
            "view_ms": {"skip": s, "never": n, "skip_all": times["skip"], "never_all": times["never"]},
            "skip_over_never_median": s["median_ms"] / n["median_ms"],
            "skip_median_inside_never_window": n["min_ms"] <= s["median_ms"] <= n["max_ms"],
            "skip_max_below_never_min": s["max_ms"] < n["min_ms"],
            "maps_bit_identical": bool(same),
            "blocks": count_blocks(r, batch, coarse, fine),
        }
        print(scene, json.dumps(result["scenes"][scene]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
