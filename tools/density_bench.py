#!/usr/bin/env python3
"""Time density queries (NeRF.get_density, nerf.py:136-143) and density + gradient queries on P points of an 8x256 view-branch
field (multires 10/4, synthetic weights, frozen parameters).  Legs per (P, precision), all in one process, alternating:

  a  the way before the density twin, kept callable here as plain code: forward(points[:, None], ones)[..., -1] -- the whole
     field with an all-ones view direction -- and, for the gradient, torch.autograd.grad of its sum with respect to the points
     (the training forward with every saved activation, then the inputs-only dX chain over the full model);
  b  get_density on the twin (trunk + alpha_linear), and density_and_grad on its two-launch route (the twin's training forward
     + its dX chain, in a workspace);
  c  density_and_grad on the fused kernel (csrc/density_grad.hip: one launch, no workspace; bf16 only).

Per leg: GPU ms per call (device events around `rounds` x `calls` calls; the legs take turns round by round, the median round
is reported with the spread), points/s, the peak of torch's allocator above the resident input (workspace + outputs), and for
leg c the algorithmic FLOP rate: 2 x MACs of the trunk and head forward plus the chain's transposed products and its two encoding
products, over the measured time.  Prints one JSON line.

    python tools/density_bench.py [--points 4096 65536 1048576] [--precision bf16 fp32_split] [--out profiles/density_query.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ.setdefault("NERF_AMD_QUIET", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nerf_shared_amd import nerf, synth  # noqa: E402

ARCH = dict(D=8, W=256, output_ch=5, skips=[4], use_viewdirs=True, multires=10, multires_views=4)
W, E = 256, 63                                     # hidden width, encoded xyz columns
# MACs per point: pts_linears.0 (E x W), six W x W layers, the skip layer ((E + W) x W), alpha_linear (W)
TRUNK_MACS = E * W + 6 * W * W + (E + W) * W + W
# the chain: alpha_linear^T, seven W x W transposed layers (the skip layer's h columns among them), and the encoding products
# through the skip layer and through pts_linears.0 (E x W each)
CHAIN_MACS = W + 7 * W * W + 2 * E * W
FULL_MACS = TRUNK_MACS + W * W + (W + 27) * (W // 2) + 3 * (W // 2)          # + feature_linear, views_linears.0, rgb_linear


def full_sigma(m, p, ones):
    return m.forward(p[:, None], ones)[..., 0, -1]


def legs_for(m, p, precision):
    ones = torch.ones(p.shape[0], 3, device=p.device)

    def a_value():
        with torch.no_grad():
            return full_sigma(m, p, ones)

    def a_grad():
        pf = p.detach().requires_grad_(True)
        s = full_sigma(m, pf, ones)
        return s, torch.autograd.grad(s.sum(), pf)[0]

    def b_value():
        with torch.no_grad():
            return m.get_density(p)

    def route(name):
        def call():
            nerf.set_density_grad_route(name)
            return m.density_and_grad(p)
        return call

    legs = {"a_value_full_field": a_value, "b_value_get_density": b_value,
            "a_grad_autograd_full_field": a_grad, "b_grad_two_launch": route("two_launch")}
    if precision == "bf16":
        legs["c_grad_fused"] = route("auto")
    return legs


def measure(legs, calls, rounds, warmup, dev):
    times = {k: [] for k in legs}
    peaks = {}
    for k, fn in legs.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = fn()
        torch.cuda.synchronize()
        peaks[k] = torch.cuda.max_memory_allocated(dev) - base
        del out
    for _ in range(rounds):                        # the legs take turns: a drifting clock or a busy neighbour hits them alike
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / calls)
    return times, peaks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[4096, 65536, 1048576])
    ap.add_argument("--precision", nargs="+", default=["bf16", "fp32_split"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-points-per-round", type=int, default=1 << 22, help="calls per round = this / P, at least 2")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("density_bench needs a ROCm device: a CPU run measures nothing")
    dev = torch.device("cuda:0")
    result = {"tool": "density_bench", "arch": ARCH, "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
              "macs_per_point": {"full_field": FULL_MACS, "trunk_and_head": TRUNK_MACS, "chain": CHAIN_MACS}, "runs": []}
    rng = np.random.default_rng(0)
    for precision in args.precision:
        m = nerf.NeRF(**ARCH)
        m.load_state_dict(synth.torch_state_dict(0, 1.0, **{**ARCH, "skips": tuple(ARCH["skips"])}))
        m.precision = precision
        m = m.to(dev).requires_grad_(False)
        for P in args.points:
            p = torch.from_numpy(rng.uniform(-2, 2, size=(P, 3)).astype(np.float32)).to(dev)
            calls = max(2, args.min_points_per_round // P)
            times, peaks = measure(legs_for(m, p, precision), calls, args.rounds, args.warmup, dev)
            run = {"points": P, "precision": precision, "calls_per_round": calls, "legs": {}}
            for k, ts in times.items():
                ms = statistics.median(ts)
                leg = {"ms": ms, "ms_min": min(ts), "ms_max": max(ts), "points_per_s": P / (ms * 1e-3), "peak_bytes": peaks[k],
                       "peak_bytes_per_point": peaks[k] / P}
                if k == "c_grad_fused":
                    leg["algorithmic_tflops"] = 2.0 * (TRUNK_MACS + CHAIN_MACS) * P / (ms * 1e-3) / 1e12
                run["legs"][k] = leg
            result["runs"].append(run)
    nerf.set_density_grad_route("auto")
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
