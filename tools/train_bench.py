#!/usr/bin/env python3
"""Time one training step of the reference's loop (main.py:67-112 without the data loader):
N_rand rays -> render (64+128, two 8x256 view-branch models) -> mse(rgb)+mse(rgb0) -> backward -> Adam.

    python tools/train_bench.py [--rays 1024] [--steps 20]
    python tools/train_bench.py --joint [--out profiles/joint_step.json] [--baseline FILE]     (learned poses: joint_bench)
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NERF_AMD_QUIET", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerf_shared_amd import nerf, render_utils, synth, utils  # noqa: E402

ARCH = dict(D=8, W=256, output_ch=5, skips=[4], use_viewdirs=True, multires=10, multires_views=4)


def _fresh_models(dev, precision):
    models = []
    for seed in (0, 10):
        m = nerf.NeRF(**ARCH)
        m.load_state_dict(synth.torch_state_dict(seed, 1.0, **{**ARCH, "skips": tuple(ARCH["skips"])}))
        m.precision = precision
        models.append(m.to(dev))
    return models


def _ms_per_call(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def joint_bench(args):
    """--joint: the captured joint step (utils.CapturedJointStep: learned poses beside the fields) against
    utils.CapturedTrainStep in ONE process on one batch shape (args.rays rays of 400 x 400 images, 64 + 128 samples), in bf16
    and fp32_split, and the two new kernel pairs alone at M = 100 poses, n = 1024 and 4096 rays.  One JSON object; --out FILE
    writes it; --baseline FILE embeds the JSON lines `train_bench.py --graph --precision P` printed at the parent commit."""
    from nerf_shared_amd import _lib, optim
    dev = torch.device("cuda:0")
    H = W = 400
    M, n = args.joint_poses, args.rays
    K = synth.lego_intrinsics(H, W)
    r = render_utils.Renderer(perturb=1.0, N_importance=128, N_samples=64, use_viewdirs=True, white_bkgd=True,
                              raw_noise_std=0.0, near=2.0, far=6.0)
    rng = np.random.default_rng(0)
    poses = utils.perturbed_start_poses(np.concatenate([synth.LEGO_C2W, [[0, 0, 0, 1]]], 0), M, 10.0, 0.2, seed=1)
    pix_np = np.stack([rng.integers(0, W, size=n), rng.integers(0, H, size=n)], -1)
    idx_np = rng.integers(0, M, size=n)
    pix, idx = torch.from_numpy(pix_np).to(dev, torch.int32), torch.from_numpy(idx_np).to(dev, torch.int32)
    target = torch.rand(n, 3, device=dev)
    out = {"rays_per_step": n, "samples": "64+128", "image": [H, W], "poses": M, "steps_per_window": args.steps, "windows": args.windows,
           "timing": "wall ms per replay over a window that ends in a device synchronise; median and min / max of the alternating windows",
           "precisions": {}}
    for precision in ("bf16", "fp32_split"):
        # three captured steps, each with models and optimizer of its own, timed in alternating windows of args.steps replays
        mc, mf = _fresh_models(dev, precision)
        opt = optim.Adam(list(mc.parameters()) + list(mf.parameters()), lr=5e-4, betas=(0.9, 0.999))
        with torch.no_grad():
            rays_t = torch.stack(utils.get_rays_indexed(H, W, K, torch.from_numpy(poses).to(dev), pix, idx), 0)
        train = utils.CapturedTrainStep(r, H, W, K, 32768, mc, mf, opt, n)        # plain training on the rays those poses give
        legs, keep = {"captured_train_step": lambda: train(rays_t, target)}, [mc, mf, opt]
        for tag, with_bank in (("captured_joint_step", False), ("captured_joint_step_with_bank_draw", True)):
            mc, mf = _fresh_models(dev, precision)
            lp = utils.LearnedPoses(poses, frozen=(0,)).to(dev)
            opt = optim.Adam([{"params": list(mc.parameters()) + list(mf.parameters()), "lr": 5e-4},
                              {"params": [lp.twist.xi], "lr": 1e-3}], betas=(0.9, 0.999))
            bank = utils.ImageBankSampler(torch.rand(M, H, W, 3, device=dev), n, seed=0) if with_bank else None
            joint = utils.CapturedJointStep(r, H, W, K, 32768, mc, mf, lp, opt, n, sampler=bank)
            legs[tag] = joint if with_bank else (lambda j=joint: j(pix, idx, target))
            keep += [mc, mf, lp, opt, bank]
        windows = {tag: [] for tag in legs}
        for w in range(args.windows):
            for tag, fn in legs.items():
                windows[tag].append(_ms_per_call(fn, args.steps, args.warmup if w == 0 else 3))
        res = {}
        for tag, ms in windows.items():
            res[tag + "_ms"] = float(np.median(ms))
            res[tag + "_ms_min_max"] = [min(ms), max(ms)]
        res["joint_over_train"] = res["captured_joint_step_ms"] / res["captured_train_step_ms"]
        out["precisions"][precision] = res
        del legs, keep, train, joint
    # the new kernel pairs alone (forward + backward per call pair), through the C entry points
    k4 = (ctypes.c_double * 4)(float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
    table = torch.from_numpy(poses).to(dev)
    xi = torch.from_numpy((0.05 * rng.normal(size=(M, 6))).astype(np.float32)).to(dev)
    T, g_T, g_xi, g_c2w = torch.empty(M, 16, device=dev), torch.rand(M, 16, device=dev), torch.empty(M, 6, device=dev), torch.empty(M, 12, device=dev)
    s = _lib.stream_of(dev)
    lib = _lib.lib

    def twist_pair():
        lib.nerf_amd_se3_exp_batch(xi.data_ptr(), table.data_ptr(), 16, M, T.data_ptr(), s)
        lib.nerf_amd_se3_exp_batch_backward(xi.data_ptr(), table.data_ptr(), 16, M, g_T.data_ptr(), g_xi.data_ptr(), s)

    out["kernel_pairs_us"] = {"poses": M, "se3_exp_batch+backward": _ms_per_call(twist_pair, 500, 20) * 1e3}
    for nn in (1024, 4096):
        p = torch.from_numpy(np.stack([rng.integers(0, W, size=nn), rng.integers(0, H, size=nn)], -1)).to(dev, torch.int32)
        i = torch.from_numpy(rng.integers(0, M, size=nn)).to(dev, torch.int32)
        o, d, g_o, g_d = (torch.rand(nn, 3, device=dev) for _ in range(4))

        def rays_pair():
            lib.nerf_amd_rays_at_pixels_indexed(H, W, k4, table.data_ptr(), 16, 4, M, p.data_ptr(), i.data_ptr(), nn, o.data_ptr(), d.data_ptr(), s)
            lib.nerf_amd_rays_at_pixels_indexed_backward(H, W, k4, p.data_ptr(), i.data_ptr(), nn, M, g_o.data_ptr(), g_d.data_ptr(),
                                                         g_c2w.data_ptr(), s)

        out["kernel_pairs_us"]["rays_at_pixels_indexed+backward n=%d" % nn] = _ms_per_call(rays_pair, 500, 20) * 1e3
    out["kernel_pairs_us"]["note"] = "wall time per enqueued pair over 500 back-to-back pairs (launch-bound: two tiny launches each)"
    if args.baseline:
        with open(args.baseline) as f:
            out["parent_commit_captured_train_step"] = [json.loads(line) for line in f if line.strip().startswith("{")]
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--joint", action="store_true", help="time utils.CapturedJointStep against utils.CapturedTrainStep (see joint_bench)")
    ap.add_argument("--joint-poses", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5, help="--joint: alternating timing windows of --steps replays per leg")
    ap.add_argument("--baseline", default=None, help="--joint: a file of train_bench.py JSON lines measured at the parent commit")
    ap.add_argument("--out", default=None, help="--joint: write the result here")
    ap.add_argument("--rays", type=int, default=1024)      # N_rand of configs/lego.txt:15
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--adam", choices=["foreach", "fused", "amd"], default="amd",
                    help="amd: nerf_shared_amd.optim.Adam (what utils.get_optimizer returns); foreach / fused: torch.optim.Adam")
    ap.add_argument("--tuning", type=int, default=0, help="nerf_amd_set_tuning(0, value): an A/B value of include/nerf_amd.h key 0 (50..58, the weight-gradient launchers of rounds 1-3, do nothing any more)")
    ap.add_argument("--precision", choices=["bf16", "fp32_split", "fp32"], default="bf16",
                    help="arithmetic of the field and of its backward pass (fp32 trains on the exact-fp32 path, csrc/train_f32.hip)")
    ap.add_argument("--netdepth", type=int, default=8, help="anything but 8 x 256 with skip 4 trains on the exact-fp32 path (csrc/train_f32.hip)")
    ap.add_argument("--netwidth", type=int, default=256)
    ap.add_argument("--skip", type=int, default=4)
    ap.add_argument("--multires", type=int, default=10)
    ap.add_argument("--multires-views", type=int, default=4, help="15 / 6: configs/stonehenge.txt:18-19")
    ap.add_argument("--graph", action="store_true", help="utils.CapturedTrainStep: the step captured in a HIP graph and replayed")
    ap.add_argument("--cprofile", action="store_true", help="print the host-side profile of the timed steps (cProfile)")
    args = ap.parse_args()
    if args.joint:
        return joint_bench(args)
    from nerf_shared_amd import _lib
    _lib.check(_lib.lib.nerf_amd_set_tuning(0, args.tuning), "set_tuning")
    dev = torch.device("cuda:0")
    ARCH.update(multires=args.multires, multires_views=args.multires_views, D=args.netdepth, W=args.netwidth, skips=[args.skip])
    models = []
    for seed in (0, 10):
        m = nerf.NeRF(**ARCH)
        m.load_state_dict(synth.torch_state_dict(seed, 1.0, **{**ARCH, "skips": tuple(ARCH["skips"])}))
        m.precision = args.precision
        models.append(m.to(dev))
    r = render_utils.Renderer(perturb=1.0, N_importance=128, N_samples=64, use_viewdirs=True, white_bkgd=True,
                              raw_noise_std=0.0, near=2.0, far=6.0)
    params = list(models[0].parameters()) + list(models[1].parameters())
    if args.adam == "amd":
        from nerf_shared_amd import optim
        opt = optim.Adam(params, lr=5e-4, betas=(0.9, 0.999))
    else:
        opt = torch.optim.Adam(params, lr=5e-4, betas=(0.9, 0.999), fused=args.adam == "fused")
    rng = np.random.default_rng(0)
    K = synth.lego_intrinsics(400, 400)
    idx = rng.choice(160000, size=args.rays, replace=False)
    ro, rd = synth.rays_np(400, 400, K, synth.LEGO_C2W, idx)
    rays = (torch.from_numpy(ro).to(dev), torch.from_numpy(rd).to(dev))
    target = torch.rand(args.rays, 3, device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        rgb, disp, acc, extras = r.render(400, 400, K, models[0], models[1], chunk=32768, rays=rays, retraw=True)
        loss = utils.img2mse(rgb, target) + utils.img2mse(extras["rgb0"], target)       # main.py:93-98
        loss.backward()
        opt.step()
        return loss

    if args.graph:
        if args.adam != "amd":
            raise SystemExit("--graph needs --adam amd")
        captured = utils.CapturedTrainStep(r, 400, 400, K, 32768, models[0], models[1], opt, args.rays)
        rays_t = torch.stack(list(rays), 0)

        def step():                                  # noqa: F811  (one replay + the loop's LR decay, main.py:108-112)
            loss = captured(rays_t, target)
            for g in opt.param_groups:
                g["lr"] = 5e-4 * (0.1 ** (captured.optimizer._together[0]["step"] / 250000.0))
            return loss

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if args.cprofile:
        import cProfile
        import pstats
        prof = cProfile.Profile()
        prof.enable()
        for _ in range(args.steps):
            step()
        prof.disable()
        torch.cuda.synchronize()
        pstats.Stats(prof).sort_stats("cumulative").print_stats(45)
        pstats.Stats(prof).sort_stats("tottime").print_stats(30)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    host = (time.perf_counter() - t0) / args.steps        # time to ENQUEUE a step: close to ms_per_step = host-bound
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    pts = args.rays * 256
    print(json.dumps({"rays_per_step": args.rays, "ms_per_step": dt * 1e3, "steps_per_s": 1 / dt,
                      "host_enqueue_ms_per_step": host * 1e3,
                      "rays_per_s": args.rays / dt, "loss": float(loss), "adam": args.adam, "precision": args.precision, "graph": bool(args.graph),
                      "model_tflops": pts * 1186816 * 3 / dt / 1e12}))


if __name__ == "__main__":
    main()
