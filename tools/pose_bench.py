#!/usr/bin/env python3
"""Time one iteration of the pose-estimation loop (examples/relative_pose_estimation_demo/demo_est_rel_pose.py:74-98): seven
pose parameters against `batch` selected pixels of a 400 x 400 view, frozen 8x256 view-branch fields, 64 + 128 samples,
synthetic weights.  Three legs per (batch, precision):

  a  the loop as it could be written before the device-side ops: the se(3) module in torch ops, utils.get_rays over the whole
     image (pose through the host), index the selected pixels, render, img2mse, backward with the weight-gradient launches
     (for this leg the tool sends the inputs-only backward through nerf_amd_field_backward), torch.optim.Adam;
  b  the device-side ops eagerly: utils.CameraTransf, utils.get_rays_at, inputs-only field backward, optim.Adam;
  c  utils.CapturedPoseStep: leg b's body captured in a HIP graph, one replay per step;
  c' leg c fed the demo's way (demo_est_rel_pose.py:75-79), what a caller had to write before the sampler: np.random.choice over
     the interest region without replacement, numpy indexing of the region and of the image, torch.Tensor(...).to(device);
  d  utils.CapturedPoseStep(sampler=utils.PixelSampler(...)): the draw and the gather are the first launch of the captured body.
Legs c' and d share one interest region of the 400 x 400 image (500 seeded points, dilated 3 times with a 5 x 5 window: 40 000 to
80 000 pixels), the batch and the models; they also record wall ms per step (enqueue the whole loop, then wait for the device).

The synthetic fields get a density bias of +1: at scale 1.0 every sigma is negative and the volume would be empty (a white
image, no pose gradient); with it the three legs' losses follow the same optimisation and can be compared.

Legs a, b and c are fed from eight prepared pixel sets (no selection cost).  Per leg: host ms per step (wall time of enqueueing the steps, no synchronisation added) and GPU ms per step (events around
the timed steps).  Prints one JSON line.

    python tools/pose_bench.py [--steps 60] [--warmup 5] [--out profiles/pose_step.json]

--multistart runs another leg INSTEAD (run_multistart): B = 1, 2, 4, 8, 16 pose hypotheses in one utils.CapturedMultiPoseStep
replay against B sequential replays of utils.CapturedPoseStep, GPU and host ms for both and their ratio per row.  Give each
invocation its own time limit (a hung device must end the run, not the next tool):

    timeout -k 10 900 python tools/pose_bench.py --multistart --out profiles/pose_multistart.json

--multistart-trace B replays one multi-step 40 times and times nothing, for a kernel timeline of the step:

    timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d /tmp/tr -- python3 tools/pose_bench.py --multistart-trace 8 --batch 512 --precision bf16
    python3 tools/step_timeline.py $(find /tmp/tr -name '*kernel_trace.csv') > profiles/pose_multistart_timeline_B8.txt
"""
import argparse
import contextlib
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NERF_AMD_QUIET", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerf_shared_amd import _lib, nerf, optim, render_utils, synth, utils  # noqa: E402

ARCH = dict(D=8, W=256, output_ch=5, skips=[4], use_viewdirs=True, multires=10, multires_views=4)
H = W = 400
LRATE = 0.01


class TorchCameraTransf(torch.nn.Module):
    """The se(3) module of leg a, from the formula in torch ops: exp_i = [[I + sin K + (1 - cos) K^2, A v], [0, 1]] with
    K = [w]x and A = theta I + (1 - cos) K + (theta - sin) K^2; T = exp_i @ x."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.normal(0., 1e-6, size=(3,)))
        self.v = torch.nn.Parameter(torch.normal(0., 1e-6, size=(3,)))
        self.theta = torch.nn.Parameter(torch.normal(0., 1e-6, size=()))

    def forward(self, x):
        w, z = self.w, torch.zeros((), device=self.w.device)
        K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
        K2, eye = K @ K, torch.eye(3, device=w.device)
        s, c = torch.sin(self.theta), torch.cos(self.theta)
        R = eye + s * K + (1 - c) * K2
        u = (self.theta * eye + (1 - c) * K + (self.theta - s) * K2) @ self.v
        bottom = torch.tensor([[0., 0., 0., 1.]], device=w.device)
        return torch.cat([torch.cat([R, u[:, None]], 1), bottom], 0) @ x


@contextlib.contextmanager
def full_backward_for_frozen_models(models):
    """Leg a only: what a backward through frozen fields cost before nerf_amd_field_backward_inputs existed -- the zeroed
    parameter-gradient buffer and nerf_amd_field_backward with its weight-gradient launches, for gradients nothing reads.
    The A/B lives here, in the tool: the binding's inputs-only entry is replaced for the duration of the leg."""
    by_handle = {m._handle.value: m for m in models}
    inputs_only = _lib.lib.nerf_amd_field_backward_inputs

    def full(handle, g_raw, pts, viewdirs, rays, ray_ch, z_vals, R, S, ws, ws_bytes, g_pts, g_rays, g_vd, prec, stream):
        m = by_handle[handle.value]
        sizes, shapes = m._grad_layout()
        n = len(shapes)
        flat = torch.zeros(sizes[-1], device=next(m.parameters()).device, dtype=torch.float32)
        wp = (ctypes.c_void_p * n)(*[flat.data_ptr() + 4 * o for o in sizes[0:n]])
        bp = (ctypes.c_void_p * n)(*[flat.data_ptr() + 4 * o for o in sizes[n:2 * n]])
        return _lib.lib.nerf_amd_field_backward(handle, g_raw, pts, viewdirs, rays, ray_ch, z_vals, R, S, ws, ws_bytes, wp, bp, n,
                                                g_pts, g_rays, g_vd, prec, stream)
    _lib.lib.nerf_amd_field_backward_inputs = full
    try:
        yield
    finally:
        _lib.lib.nerf_amd_field_backward_inputs = inputs_only


def timed(step, steps, warmup, wall=False):
    for k in range(warmup):
        step(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for k in range(steps):
        loss = step(warmup + k)
    host = (time.perf_counter() - t0) / steps
    e1.record()
    torch.cuda.synchronize()
    total = (time.perf_counter() - t0) / steps
    out = {"host_ms_per_step": host * 1e3, "gpu_ms_per_step": e0.elapsed_time(e1) / steps, "loss": float(loss.detach())}
    if wall:
        out["wall_ms_per_step"] = total * 1e3
    return out


def interest_points(n=500, seed=0):
    """Seeded stand-ins for a detector's points, [n, 2] (x, y): the region they give is the same in every run."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(H * W, size=n, replace=False)
    return np.stack([idx % W, idx // W], -1)


def draw_kernel_us(sampler, draws=100, repeats=3):
    """GPU time of one sampler.draw() (the draw / gather launch and the counter's one-thread launch), from events around a
    graph of `draws` of them; the counter is put back."""
    before = sampler.draw_count.clone()
    side = torch.cuda.Stream(sampler.pixels.device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sampler.draw()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(draws):
            sampler.draw()
    best = None
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / draws * 1e3
        best = t if best is None else min(best, t)
    sampler.draw_count.copy_(before)
    return best


def scene(dev, batch, precision):
    """Frozen models, renderer, intrinsics, the start pose and eight prepared (pixels, target) sets: what every leg runs on."""
    models = []
    for seed in (0, 10):
        m = nerf.NeRF(**ARCH)
        m.load_state_dict(synth.torch_state_dict(seed, 1.0, **{**ARCH, "skips": tuple(ARCH["skips"])}))
        m.precision = precision
        with torch.no_grad():
            m.alpha_linear.bias += 1.0            # a fog with structure instead of an empty volume (module docstring)
        models.append(m.to(dev).requires_grad_(False))
    r = render_utils.Renderer(perturb=0.0, N_importance=128, N_samples=64, use_viewdirs=True, white_bkgd=True,
                              raw_noise_std=0.0, near=2.0, far=6.0)
    K = synth.lego_intrinsics(H, W)
    start = torch.from_numpy(np.concatenate([synth.LEGO_C2W, np.array([[0, 0, 0, 1]], np.float32)], 0)).to(dev)
    rng = np.random.default_rng(0)
    sets = []
    for _ in range(8):                        # the demo draws a new subset every iteration
        idx = rng.choice(H * W, size=batch, replace=False)
        sets.append((torch.from_numpy(np.stack([idx % W, idx // W], -1)).to(dev), torch.rand(batch, 3, device=dev)))
    return models, r, K, start, sets


def run(dev, batch, precision, steps, warmup):
    models, r, K, start, sets = scene(dev, batch, precision)

    def decay(opt, k):
        for g in opt.param_groups:
            g["lr"] = LRATE * (0.8 ** ((k + 1) / 100))

    out = {}
    # a: before the device-side ops
    torch.manual_seed(0)
    cam_a = TorchCameraTransf().to(dev)
    opt_a = torch.optim.Adam(cam_a.parameters(), lr=LRATE, betas=(0.9, 0.999))

    def step_a(k):
        pix, tgt = sets[k % len(sets)]
        opt_a.zero_grad()
        pose = cam_a(start)
        ro, rd = utils.get_rays(H, W, K, pose)
        rays = torch.stack([ro[pix[:, 1], pix[:, 0]], rd[pix[:, 1], pix[:, 0]]], 0)
        rgb = r.render_from_rays(H, W, K, 32768, rays, models[0], models[1], retraw=True)[0]
        loss = utils.img2mse(rgb, tgt)
        loss.backward()
        opt_a.step()
        decay(opt_a, k)
        return loss
    for m in models:
        m._ensure_handle(dev)
    with full_backward_for_frozen_models(models):
        out["a_get_rays_then_index"] = timed(step_a, steps, warmup)

    # b: the device-side ops, eagerly
    torch.manual_seed(0)
    cam_b = utils.CameraTransf().to(dev)
    opt_b = optim.Adam(cam_b.parameters(), lr=LRATE, betas=(0.9, 0.999))

    def step_b(k):
        pix, tgt = sets[k % len(sets)]
        opt_b.zero_grad()
        ro, rd = utils.get_rays_at(H, W, K, cam_b(start), pix)
        rgb = r.render_from_rays(H, W, K, 32768, torch.stack([ro, rd], 0), models[0], models[1], retraw=True)[0]
        loss = utils.img2mse(rgb, tgt)
        loss.backward()
        opt_b.step()
        decay(opt_b, k)
        return loss
    out["b_device_ops_eager"] = timed(step_b, steps, warmup)

    # c: captured
    torch.manual_seed(0)
    cam_c = utils.CameraTransf().to(dev)
    opt_c = optim.Adam(cam_c.parameters(), lr=LRATE, betas=(0.9, 0.999))
    captured = utils.CapturedPoseStep(r, H, W, K, 32768, models[0], models[1], cam_c, start, opt_c, batch)

    def step_c(k):
        loss = captured(*sets[k % len(sets)])
        decay(opt_c, k)
        return loss
    out["c_captured_pose_step"] = timed(step_c, steps, warmup)

    # c': the captured step fed the demo's way (host selection, two host-to-device copies per step)
    obs_img = (np.random.default_rng(1).integers(0, 256, size=(H, W, 3)).astype(np.uint8) / 255.).astype(np.float32)
    points = interest_points()
    sampler = utils.PixelSampler(obs_img, batch, strategy="interest_region", points=points, kernel_size=5, dil_iter=3, seed=0, device=dev)
    interest_regions = sampler.region.cpu().numpy()
    torch.manual_seed(0)
    cam_h = utils.CameraTransf().to(dev)
    opt_h = optim.Adam(cam_h.parameters(), lr=LRATE, betas=(0.9, 0.999))
    captured_h = utils.CapturedPoseStep(r, H, W, K, 32768, models[0], models[1], cam_h, start, opt_h, batch)
    np.random.seed(0)

    def step_h(k):
        rand_inds = np.random.choice(interest_regions.shape[0], size=batch, replace=False)
        sel = interest_regions[rand_inds]
        target_s = torch.Tensor(obs_img[sel[:, 1], sel[:, 0]]).to(dev)
        loss = captured_h(sel, target_s)
        decay(opt_h, k)
        return loss
    out["c_prime_captured_host_selection"] = timed(step_h, steps, warmup, wall=True)

    # d: the captured step that draws its own pixels
    torch.manual_seed(0)
    cam_d = utils.CameraTransf().to(dev)
    opt_d = optim.Adam(cam_d.parameters(), lr=LRATE, betas=(0.9, 0.999))
    captured_d = utils.CapturedPoseStep(r, H, W, K, 32768, models[0], models[1], cam_d, start, opt_d, batch, sampler=sampler)

    def step_d(k):
        loss = captured_d()
        decay(opt_d, k)
        return loss
    out["d_captured_with_sampler"] = timed(step_d, steps, warmup, wall=True)
    out["region_pixels"] = sampler.M
    out["draw_us_per_call"] = draw_kernel_us(sampler)
    return out


MULTISTART_B = (1, 2, 4, 8, 16)


def window(step, steps):
    """(host ms, GPU ms) per call of `step` over `steps` calls: wall time of the enqueue, events around the window."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for k in range(steps):
        step(k)
    host = (time.perf_counter() - t0) / steps
    e1.record()
    torch.cuda.synchronize()
    return host * 1e3, e0.elapsed_time(e1) / steps


def run_multistart(dev, batch, precision, steps, warmup, repeats):
    """The multi-start leg: per B, one replay of utils.CapturedMultiPoseStep (B hypotheses around the start pose, B * batch
    rays to every field kernel) against B sequential replays of the existing utils.CapturedPoseStep -- the yardstick, what a
    caller runs without the multi-step -- in the same process, on the same pixel sets.  Both are warmed up, then timed in
    `repeats` alternating windows of `steps` steps; the medians are reported with the extremes of the windows."""
    models, r, K, start, sets = scene(dev, batch, precision)

    def decay(opt, k):
        for g in opt.param_groups:
            g["lr"] = LRATE * (0.8 ** ((k + 1) / 100))

    torch.manual_seed(0)
    cam = utils.CameraTransf().to(dev)
    opt = optim.Adam(cam.parameters(), lr=LRATE, betas=(0.9, 0.999))
    single = utils.CapturedPoseStep(r, H, W, K, 32768, models[0], models[1], cam, start, opt, batch)
    rows = []
    for B in MULTISTART_B:
        starts = torch.from_numpy(utils.perturbed_start_poses(start.cpu().numpy(), B, 5.0, 0.1, seed=0)).to(dev)
        torch.manual_seed(0)
        cams = utils.CameraTransfBatch(B).to(dev)
        opt_m = optim.Adam(cams.parameters(), lr=LRATE, betas=(0.9, 0.999))
        multi = utils.CapturedMultiPoseStep(r, H, W, K, max(32768, B * batch), models[0], models[1], cams, starts, opt_m, batch)

        def step_multi(k):
            multi(*sets[k % len(sets)])
            decay(opt_m, k)

        def step_sequential(k):
            for _ in range(B):                    # B hypotheses, one after another (each its own replay and pixel copy)
                single(*sets[k % len(sets)])
            decay(opt, k)

        for k in range(warmup):
            step_multi(k)
            step_sequential(k)
        m, q = [], []
        for _ in range(repeats):
            m.append(window(step_multi, steps))
            q.append(window(step_sequential, steps))
        med = lambda v: float(np.median(v))          # noqa: E731
        row = {"precision": precision, "batch": batch, "B": B,
               "multi_gpu_ms": med([x[1] for x in m]), "multi_host_ms": med([x[0] for x in m]),
               "sequential_gpu_ms": med([x[1] for x in q]), "sequential_host_ms": med([x[0] for x in q]),
               "multi_gpu_ms_min_max": [min(x[1] for x in m), max(x[1] for x in m)],
               "sequential_gpu_ms_min_max": [min(x[1] for x in q), max(x[1] for x in q)],
               "losses_finite": bool(torch.isfinite(multi.losses).all())}
        row["sequential_over_multi_gpu"] = row["sequential_gpu_ms"] / row["multi_gpu_ms"]
        row["sequential_over_multi_host"] = row["sequential_host_ms"] / row["multi_host_ms"]
        rows.append(row)
        print("multistart %s batch %d B %2d: multi %.3f ms GPU (%.3f host), %d sequential %.3f ms GPU (%.3f host), ratio %.2f"
              % (precision, batch, B, row["multi_gpu_ms"], row["multi_host_ms"], B, row["sequential_gpu_ms"], row["sequential_host_ms"],
                 row["sequential_over_multi_gpu"]), file=sys.stderr, flush=True)
        del multi, cams, opt_m
    return rows


def trace_multistart(args):
    """--multistart-trace B: nothing is timed; 40 replays of one CapturedMultiPoseStep (first --batch, first --precision) for a
    profiler to look at (tools/step_timeline.py prints the kernels of the last two steps)."""
    dev = torch.device("cuda:0")
    B, batch = args.multistart_trace, args.batch[0]
    models, r, K, start, sets = scene(dev, batch, args.precision[0])
    starts = torch.from_numpy(utils.perturbed_start_poses(start.cpu().numpy(), B, 5.0, 0.1, seed=0)).to(dev)
    torch.manual_seed(0)
    cams = utils.CameraTransfBatch(B).to(dev)
    opt = optim.Adam(cams.parameters(), lr=LRATE, betas=(0.9, 0.999))
    multi = utils.CapturedMultiPoseStep(r, H, W, K, max(32768, B * batch), models[0], models[1], cams, starts, opt, batch)
    for k in range(40):
        multi(*sets[k % len(sets)])
    torch.cuda.synchronize()
    print(json.dumps({"tool": "pose_bench --multistart-trace", "B": B, "batch": batch, "precision": args.precision[0],
                      "losses": [float(v) for v in multi.losses.cpu()]}))


def main_multistart(args):
    dev = torch.device("cuda:0")
    steps = max(args.steps, 100)
    result = {"tool": "pose_bench --multistart", "image": [H, W], "samples": [64, 128], "steps_per_window": steps, "windows": args.repeats,
              "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "hypotheses": list(MULTISTART_B),
              "sequential": "ONE utils.CapturedPoseStep object (one module, one start pose) replayed B times per step, each replay with "
                            "its own copy of the pixel set: the time of B single-hypothesis steps, not B distinct hypotheses",
              "multi": "one replay of utils.CapturedMultiPoseStep (B distinct hypotheses around the start pose)", "rows": []}
    for precision in args.precision:
        for batch in args.batch:
            result["rows"] += run_multistart(dev, batch, precision, steps, args.warmup, args.repeats)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--multistart", action="store_true",
                    help="run the multi-start leg alone: CapturedMultiPoseStep for B in 1..16 against B sequential CapturedPoseStep "
                         "replays (profiles/pose_multistart.json)")
    ap.add_argument("--multistart-trace", type=int, default=0, metavar="B",
                    help="replay one CapturedMultiPoseStep of B hypotheses 40 times and time nothing (run it under a profiler)")
    ap.add_argument("--repeats", type=int, default=5, help="--multistart: alternating timed windows per row")
    ap.add_argument("--steps", type=int, default=60, help="timed steps per leg (>= 50)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, nargs="+", default=[256, 512])          # the demo's --batch_size default is 512
    ap.add_argument("--precision", nargs="+", default=["bf16", "fp32_split"])
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.multistart_trace:
        return trace_multistart(args)
    if args.multistart:
        return main_multistart(args)
    dev = torch.device("cuda:0")
    result = {"tool": "pose_bench", "image": [H, W], "samples": [64, 128], "steps": args.steps, "warmup": args.warmup,
              "device": torch.cuda.get_device_name(0), "runs": []}
    for precision in args.precision:
        for batch in args.batch:
            result["runs"].append({"batch": batch, "precision": precision, **run(dev, batch, precision, args.steps, args.warmup)})
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
