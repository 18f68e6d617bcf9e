#!/usr/bin/env python3
"""Same-process A/B of whole-view renders (the bench's workload: 400x400, 64+128, 8x256 with view branch) under two
values of nerf_amd_set_tuning(0, .): interleaved rounds, bit-identical outputs required.  KEY:VALUE names another tuning key;
across values of key 2 (feature_linear folded into views_linears.0: 2:1 = unfolded, 2:0 = folded in the render path) disp
and acc must be bit-identical and the rgb difference is printed.

    python tools/micro/view_ab.py 0 44 42     # 44: the fine-pass field kernels on a stream of their own; 42: static tile deal
    python tools/micro/view_ab.py 2:1 2:0 --out profiles/view_fold_ab.json
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
os.environ.setdefault("NERF_AMD_QUIET", "1")
import torch  # noqa: E402

from nerf_shared_amd import _lib, nerf, render_utils, synth  # noqa: E402

ARCH = dict(D=8, W=256, output_ch=5, skips=[4], use_viewdirs=True, multires=10, multires_views=4)


def main():
    argv = sys.argv[1:]
    out_path = None
    if "--out" in argv:
        i = argv.index("--out")
        out_path = argv[i + 1]
        del argv[i:i + 2]
    variants = [tuple(int(x) for x in v.split(":")) if ":" in v else (0, int(v)) for v in argv] or [(0, 0), (0, 44)]
    dev = torch.device("cuda:0")
    ms = []
    for seed in (1, 19):
        m = nerf.NeRF(**ARCH)
        m.load_state_dict(synth.torch_state_dict(seed, 3.0, **{**ARCH, "skips": (4,)}))
        ms.append(m.to(dev).requires_grad_(False))
    r = render_utils.Renderer(perturb=0.0, N_importance=128, N_samples=64, use_viewdirs=True, white_bkgd=True, raw_noise_std=0.0, near=2.0, far=6.0)
    K = synth.lego_intrinsics(400, 400)
    c2w = torch.from_numpy(synth.LEGO_C2W)
    times = {v: [] for v in variants}
    outs = {}
    with torch.no_grad():
        for rnd in range(12):
            for v in variants:
                _lib.check(_lib.lib.nerf_amd_set_tuning(*v), "tuning")
                for _ in range(2):
                    r.render(400, 400, K, ms[0], ms[1], chunk=32768, c2w=c2w, retraw=False)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(5):
                    out = r.render(400, 400, K, ms[0], ms[1], chunk=32768, c2w=c2w, retraw=False)
                b.record()
                torch.cuda.synchronize()
                times[v].append(a.elapsed_time(b) / 5)
                outs[v] = [t.clone() for t in out[:3]]
    for key in (0, 2):
        _lib.lib.nerf_amd_set_tuning(key, 0)
    report = {}
    for v in variants:
        t = times[v]
        print("tuning %d:%-3d median %.3f ms per view, best %.3f, worst %.3f" % (v + (statistics.median(t), min(t), max(t))))
        report["%d:%d" % v] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "spread_ms": max(t) - min(t),
                               "rounds": len(t)}
    ref = outs[variants[0]]
    same = lambda x, y: torch.equal(torch.nan_to_num(x), torch.nan_to_num(y))       # noqa: E731
    for v in variants[1:]:
        if v[0] == 2 or variants[0][0] == 2:          # (rgb, disp, acc): the fold moves rgb only
            ok = same(ref[1], outs[v][1]) and same(ref[2], outs[v][2])
            d = float((ref[0] - outs[v][0]).abs().max())
            print("tuning %d:%d disp and acc bit-identical to %d:%d: %s; max |rgb difference| %.3e" % (v + variants[0] + (ok, d)))
            report["%d:%d_vs_%d:%d" % (v + variants[0])] = {"disp_acc_bit_identical": ok, "rgb_max_abs_diff": d}
        else:
            ok = all(same(x, y) for x, y in zip(ref, outs[v]))
            print("tuning %d:%d bit-identical to %d:%d: %s" % (v + variants[0] + (ok,)))
            report["%d:%d_vs_%d:%d" % (v + variants[0])] = {"bit_identical": ok}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
