"""GPU tests (-m gpu) of the split-precision backward pass (precision "fp32_split": csrc/mlp_split.hip SAVE,
mlp_bwd_split.hip, backward.hip dw2s_body) and of the fused family's "fp32" training (the exact-fp32 path, csrc/train_f32.hip)
against torch.autograd on the PLAIN fp32 oracle -- no rounding model.

The reference trains and pose-optimises in fp32 (main.py:85-104, demo_est_rel_pose.py:87-98); these are the gates that say
the build does too: relative L2 <= 1e-3 and cosine >= 0.9999 for every parameter tensor and for the ray gradients
(measured: 1e-6 ... 2e-5, the distance fp64 autograd keeps from fp32 autograd on the same inputs).

One thing is NOT left to chance in the two-pass tests: the fine pass's depths.  sample_pdf divides by bin masses as small as
1e-5 (utils.py:110-113), so a last-bit difference in the coarse weights moves a few fine samples by a bin width, and the
fine network's gradients with them -- fp64 autograd of the oracle itself sits 2.5e-3 from its fp32 autograd end to end
(tools/experiments/split_bwd_sim.py).  The depths are constants of the gradient (render_utils.py:145 detaches them), so the
oracle evaluates its fine pass on the depths the GPU run produced (which test_gpu_split.py / the staged tests check on their
own); the end-to-end comparison on the oracle's own depths is reported beside it with the looser gate that floor allows.
"""
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
pytestmark = pytest.mark.gpu

from nerf_shared_amd import synth  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402
from test_gpu_backward import BASE, NOVD, NOVD4, NOVD15, VD, VD15, _batch, rel_err, sphere_run  # noqa: E402,F401

GATE_REL, GATE_COS = 1e-3, 0.9999


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def cosine(a, b):
    a, b = a.detach().cpu().double().flatten(), b.detach().cpu().double().flatten()
    return float(a @ b / (a.norm() * b.norm()).clamp_min(1e-300))


def models(dev, seed, sharpen, arch, precision):
    from nerf_shared_amd import nerf
    sd = synth.torch_state_dict(seed, sharpen, **{**arch, "skips": (4,)})
    m = nerf.NeRF(**arch)
    m.load_state_dict(sd)
    m = m.to(dev)
    m.precision = precision
    cpu = {k: v.clone().requires_grad_(True) for k, v in O.state_dict_to_torch(sd).items()}
    return m, cpu


def check_params(tag, m, cpu, table):
    for name, p in m.named_parameters():
        if cpu[name].grad is None:               # views_linears.0 of an output_linear model: unused there too (nerf.py:83)
            assert p.grad is None, name
            continue
        assert p.grad is not None and p.grad.shape == cpu[name].shape, name
        g = p.grad.detach().cpu()
        assert torch.isfinite(g).all(), name
        table.append((tag + name, rel_err(g, cpu[name].grad), cosine(g, cpu[name].grad)))


def assert_table(table, gate_rel=GATE_REL, gate_cos=GATE_COS):
    for row in table:
        print("%-40s rel-L2 vs fp32 autograd %.3e   cos %.8f" % row)
    for name, e, c in table:
        assert e < gate_rel and c > gate_cos, (name, e, c)


FIELD_CASES = [(0, 1.0, VD), (1, 2.0, VD), (2, 1.0, VD15), (3, 1.0, NOVD), (4, 2.0, NOVD4), (5, 1.0, NOVD15)]
FIELD_IDS = ["vd_s0", "vd_x2", "vd_15_6", "novd", "novd_out4_x2", "novd_15_out13"]


def field_run(dev, seed, sharpen, arch, precision):
    """NeRF.forward under autograd for a random linear loss on raw (70 rays x 13 samples: 910 points, ragged), and the
    same on the fp32 oracle: (model, oracle state with gradients, training forward's raw, oracle raw, pts, vd)."""
    rng = np.random.default_rng(11)
    R, S = 70, 13
    pts = torch.from_numpy(rng.uniform(-2, 2, size=(R, S, 3)).astype(np.float32))
    vd = torch.from_numpy(rng.normal(size=(R, 3)).astype(np.float32))
    vd = vd / vd.norm(dim=-1, keepdim=True)
    if not arch["use_viewdirs"]:
        vd = None
    coef = torch.from_numpy(rng.normal(size=(R, S, 4 if arch["use_viewdirs"] else arch["output_ch"])).astype(np.float32))
    m, cpu = models(dev, seed, sharpen, arch, precision)
    ref = O.nerf_forward(cpu, O.Arch(**arch), pts, vd)
    (ref * coef).sum().backward()
    out = m(pts.to(dev), vd.to(dev) if vd is not None else None)
    assert out.requires_grad
    (out * coef.to(dev)).sum().backward()
    return m, cpu, out, ref, pts, vd


@pytest.mark.parametrize("precision", ["fp32_split"])
@pytest.mark.parametrize("seed,sharpen,arch", FIELD_CASES, ids=FIELD_IDS)
def test_field_backward_matches_fp32_autograd(dev, seed, sharpen, arch, precision):
    """dL/dtheta of NeRF.forward for a random linear loss on raw, every architecture the training kernels cover, against
    torch.autograd on the fp32 oracle.  The training forward's values pass the fp32 forward gate and are bit-identical to
    the split-precision inference kernel's.  ('fp32' trains on the exact-fp32 path:
    test_fp32_field_backward_on_the_exact_path_matches_fp32_autograd.)"""
    m, cpu, out, ref, pts, vd = field_run(dev, seed, sharpen, arch, precision)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=1e-4, rtol=1e-4)
    with torch.no_grad():
        m.precision = "fp32_split"
        torch.testing.assert_close(m(pts.to(dev), vd.to(dev) if vd is not None else None), out.detach(), rtol=0, atol=0)
    table = []
    check_params("", m, cpu, table)
    assert_table(table)


@pytest.mark.parametrize("seed,sharpen,arch", FIELD_CASES, ids=FIELD_IDS)
def test_fp32_field_backward_on_the_exact_path_matches_fp32_autograd(dev, seed, sharpen, arch):
    """The same in 'fp32', which trains on the exact-fp32 path (csrc/train_f32.hip, NeRF._train_precision) on every
    architecture: the training forward passes the fp32 forward gate and is bit-identical to the model's own 'fp32' inference
    output (the exact kernel: train_f32's forward is mlp_fp32.hip's layer loop), and the gradients pass the exact path's gate,
    2e-5 relative L2 (test_gpu_train_f32.py), not the split gate."""
    m, cpu, out, ref, pts, vd = field_run(dev, seed, sharpen, arch, "fp32")
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=1e-4, rtol=1e-4)
    with torch.no_grad():
        inference = m(pts.to(dev), vd.to(dev) if vd is not None else None)
    torch.testing.assert_close(inference, out.detach(), rtol=0, atol=0)
    table = []
    check_params("", m, cpu, table)
    assert_table(table, gate_rel=2e-5)


def oracle_two_pass(cfg, batch, coarse, fine, z_fine, pytest_draws=False):
    """The oracle's render_rays (render_utils.py:67-174) with the fine pass evaluated on given depths: rgb0 from the coarse
    pass, rgb_map from `fine` at z_fine.  batch [N, 8|11] may carry autograd history.  pytest_draws: the reference's seeded
    jitter / sigma-noise draws (render_utils.py:124-127, :267-270), as Renderer.render_rays(pytest=True) makes them."""
    rc = O.RenderCfg(**cfg)
    n = batch.shape[0]
    rays_o, rays_d, viewdirs = batch[:, 0:3], batch[:, 3:6], (batch[:, 8:11] if batch.shape[1] > 8 else None)
    near, far = batch[:, 6:7], batch[:, 7:8]
    t_rand = O.pytest_uniform([n, rc.N_samples]) if (pytest_draws and rc.perturb > 0.0) else None
    z = O.coarse_z_vals(rc, near, far, n, t_rand)
    noise = (lambda shape: O.pytest_uniform(shape) * rc.raw_noise_std) if (pytest_draws and rc.raw_noise_std > 0.0) else (lambda shape: None)
    pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., :, None]
    raw = O.nerf_forward(coarse[0], coarse[1], pts, viewdirs)
    rgb0 = O.raw2outputs(raw, z, rays_d, rc.white_bkgd, noise(list(z.shape)))[0]
    pts = rays_o[..., None, :] + rays_d[..., None, :] * z_fine[..., :, None]
    raw = O.nerf_forward(fine[0], fine[1], pts, viewdirs)
    return O.raw2outputs(raw, z_fine, rays_d, rc.white_bkgd, noise(list(z_fine.shape)))[0], rgb0


@pytest.mark.parametrize("arch", [VD, NOVD], ids=["viewdirs", "output_linear"])
def test_training_step_gradients_match_fp32_autograd(dev, arch):
    """The reference's training loss (main.py:85-98: mse(rgb) + mse(rgb0)) through Renderer.render_rays in split precision:
    parameter gradients of both networks against fp32 autograd on the oracle (fine pass on the run's own depths, see the
    module docstring), and the end-to-end comparison on the oracle's own depths beside it."""
    from nerf_shared_amd import render_utils
    batch, target = _batch(96, 3)
    vdirs = bool(arch["use_viewdirs"])
    if not vdirs:
        batch = batch[:, :8].contiguous()
    cfg = dict(BASE, N_samples=32, N_importance=48, use_viewdirs=vdirs)
    r = render_utils.Renderer(**cfg)
    mc, cc = models(dev, 1, 2.0, arch, "fp32_split")
    mf, cf = models(dev, 11, 2.0, arch, "fp32_split")
    out = r.render_rays(batch.to(dev), mc, mf, retweights=True)
    assert out["rgb_map"].requires_grad and out["rgb0"].requires_grad and not out["z_std"].requires_grad
    t = target.to(dev)
    loss = ((out["rgb_map"] - t) ** 2).mean() + ((out["rgb0"] - t) ** 2).mean()
    loss.backward()
    # (a) the oracle on the run's own fine depths
    z_f = out["z_vals"].detach().cpu()
    rgb, rgb0 = oracle_two_pass(cfg, batch, (cc, O.Arch(**arch)), (cf, O.Arch(**arch)), z_f)
    l32 = ((rgb - target) ** 2).mean() + ((rgb0 - target) ** 2).mean()
    l32.backward()
    assert abs(float(loss) - float(l32)) < 2e-6 * max(1.0, abs(float(l32)))
    table = []
    check_params("coarse.", mc, cc, table)
    check_params("fine.", mf, cf, table)
    assert_table(table)
    # (b) end to end, the oracle resampling from its own coarse weights: the coarse network is untouched by that; the fine
    # network inherits sample_pdf's conditioning (fp64 autograd of the oracle is 2.5e-3 from fp32 here)
    c2 = {k: v.detach().clone().requires_grad_(True) for k, v in cc.items()}
    f2 = {k: v.detach().clone().requires_grad_(True) for k, v in cf.items()}
    o = O.render_rays(O.RenderCfg(**cfg), batch, (c2, O.Arch(**arch)), (f2, O.Arch(**arch)))
    (((o["rgb_map"] - target) ** 2).mean() + ((o["rgb0"] - target) ** 2).mean()).backward()
    e2e = []
    check_params("e2e.coarse.", mc, c2, e2e)
    assert_table(e2e)
    e2e_f = []
    check_params("e2e.fine.", mf, f2, e2e_f)
    assert_table(e2e_f, gate_rel=2e-2, gate_cos=0.999)


def test_ray_gradients_for_pose_estimation_match_fp32_autograd(dev):
    """dL/d(rays_o, rays_d) with frozen networks -- what the pose-estimation demo differentiates
    (demo_est_rel_pose.py:87-98): through the view-direction normalisation, both positional encodings, pts = o + d z, the
    fields and the compositing (dists scale with |d|) -- against fp32 autograd on the oracle: relative L2 <= 1e-3, cosine
    >= 0.9999 (the bf16 kernels reach cosine 0.92 here)."""
    from nerf_shared_amd import render_utils
    batch, target = _batch(80, 7)
    cfg = dict(BASE, N_samples=32, N_importance=48)
    r = render_utils.Renderer(**cfg)
    mc, cc = models(dev, 1, 2.0, VD, "fp32_split")
    mf, cf = models(dev, 11, 2.0, VD, "fp32_split")
    mc.requires_grad_(False)
    mf.requires_grad_(False)

    def assemble(o, d):                            # Renderer.render's batch assembly (render_utils.py:205-226)
        vdir = d / torch.norm(d, dim=-1, keepdim=True)
        return torch.cat([o, d, 2.0 * torch.ones_like(d[:, :1]), 6.0 * torch.ones_like(d[:, :1]), vdir], -1)

    ro = batch[:, 0:3].clone().to(dev).requires_grad_(True)
    rd = (batch[:, 3:6] * 1.3).clone().to(dev).requires_grad_(True)     # not unit length: the |d| path matters
    out = r.render_rays(assemble(ro, rd), mc, mf, retweights=True)
    t = target.to(dev)
    (((out["rgb_map"] - t) ** 2).mean() + ((out["rgb0"] - t) ** 2).mean()).backward()
    assert ro.grad is not None and rd.grad is not None and all(p.grad is None for p in mc.parameters())
    o = batch[:, 0:3].clone().requires_grad_(True)
    d = (batch[:, 3:6] * 1.3).clone().requires_grad_(True)
    frozen = lambda sd: {k: v.detach() for k, v in sd.items()}     # noqa: E731
    rgb, rgb0 = oracle_two_pass(cfg, assemble(o, d), (frozen(cc), O.Arch(**VD)), (frozen(cf), O.Arch(**VD)), out["z_vals"].detach().cpu())
    (((rgb - target) ** 2).mean() + ((rgb0 - target) ** 2).mean()).backward()
    table = [("rays_o", rel_err(ro.grad, o.grad), cosine(ro.grad, o.grad)), ("rays_d", rel_err(rd.grad, d.grad), cosine(rd.grad, d.grad))]
    assert_table(table)
    # the same through Renderer.render(rays=...) (chunked, the reference's entry point): equal to the single call
    ro2 = batch[:, 0:3].clone().to(dev).requires_grad_(True)
    rd2 = (batch[:, 3:6] * 1.3).clone().to(dev).requires_grad_(True)
    rgb_r, _, _, extras = r.render(400, 400, None, mc, mf, chunk=32, rays=(ro2, rd2), retraw=False)
    (((rgb_r - t) ** 2).mean() + ((extras["rgb0"] - t) ** 2).mean()).backward()
    assert rel_err(ro2.grad, ro.grad) < 1e-5 and rel_err(rd2.grad, rd.grad) < 1e-5


@pytest.mark.parametrize("arch", [VD, VD15], ids=["multires10_4", "multires15_6"])
def test_point_gradients_of_the_field_match_fp32_autograd(dev, arch):
    """NeRF.forward(inputs, viewdirs) with inputs / viewdirs requiring grad (frozen parameters)."""
    rng = np.random.default_rng(21)
    pts = torch.from_numpy(rng.uniform(-2, 2, size=(40, 9, 3)).astype(np.float32))
    vd = torch.from_numpy(rng.normal(size=(40, 3)).astype(np.float32))
    coef = torch.from_numpy(rng.normal(size=(40, 9, 4)).astype(np.float32))
    m, cpu = models(dev, 1, 2.0, arch, "fp32_split")
    m.requires_grad_(False)
    p_gpu, v_gpu = pts.to(dev).requires_grad_(True), vd.to(dev).requires_grad_(True)
    (m(p_gpu, v_gpu) * coef.to(dev)).sum().backward()
    p_cpu, v_cpu = pts.clone().requires_grad_(True), vd.clone().requires_grad_(True)
    (O.nerf_forward({k: v.detach() for k, v in cpu.items()}, O.Arch(**arch), p_cpu, v_cpu) * coef).sum().backward()
    assert_table([("pts", rel_err(p_gpu.grad, p_cpu.grad), cosine(p_gpu.grad, p_cpu.grad)),
                  ("viewdirs", rel_err(v_gpu.grad, v_cpu.grad), cosine(v_gpu.grad, v_cpu.grad))])


def test_adam_trajectory_follows_the_fp32_oracle(dev):
    """12 optimizer steps on a fixed batch (the loop of main.py:67-112 without the data loader) in split precision, with the
    library's Adam: the loss trajectory stays within 1e-3 (relative) of the same loop on the fp32 CPU oracle."""
    from nerf_shared_amd import optim, render_utils, utils
    batch, _ = _batch(256, 4)
    target = torch.full((256, 3), 0.25)
    cfg = dict(BASE, N_samples=32, N_importance=32)
    r = render_utils.Renderer(**cfg)
    mc, cc = models(dev, 0, 1.0, VD, "fp32_split")
    mf, cf = models(dev, 10, 1.0, VD, "fp32_split")
    opt = optim.Adam(list(mc.parameters()) + list(mf.parameters()), lr=5e-4, betas=(0.9, 0.999))
    losses = []
    b, t = batch.to(dev), target.to(dev)
    for _ in range(12):
        opt.zero_grad()
        rgb, disp, acc, extras = r.render(400, 400, None, mc, mf, chunk=128, rays=(b[:, 0:3], b[:, 3:6]), retraw=True)
        loss = utils.img2mse(rgb, t) + utils.img2mse(extras["rgb0"], t)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    opt2 = torch.optim.Adam(list(cc.values()) + list(cf.values()), lr=5e-4, betas=(0.9, 0.999))
    ocfg = O.RenderCfg(**cfg)
    ref = []
    for _ in range(12):
        opt2.zero_grad()
        o = O.render_rays(ocfg, batch, (cc, O.Arch(**VD)), (cf, O.Arch(**VD)))
        l = ((o["rgb_map"] - target) ** 2).mean() + ((o["rgb0"] - target) ** 2).mean()
        l.backward()
        opt2.step()
        ref.append(float(l))
    print("split ", ["%.6f" % v for v in losses])
    print("oracle", ["%.6f" % v for v in ref])
    assert all(y < x for x, y in zip(losses, losses[1:]))
    np.testing.assert_allclose(losses, ref, rtol=1e-3)
    # the parameters themselves after the 12 steps
    worst = max(rel_err(p, cc[n]) for n, p in mc.named_parameters())
    print("coarse parameters after 12 steps: worst rel-L2 vs oracle %.2e" % worst)
    assert worst < 1e-3


def _pose(w, dt, c2w0):
    """exp(w^) R0 | t0 + dt, torch ops only (the same function serves the GPU run and the CPU oracle).  torch.matrix_exp, not
    Rodrigues' formula through w / |w|: the derivative of that with respect to a small w cancels catastrophically in fp32
    (1e-3 between two fp32 evaluations that differ in the last bit of a sine), which would measure the test, not the library."""
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    Wx = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    return torch.cat([torch.matrix_exp(Wx) @ c2w0[:3, :3], (c2w0[:3, 3] + dt)[:, None]], 1)


_POSE_CACHE = {}


@pytest.mark.parametrize("precision", ["fp32_split", "bf16"])
def test_pose_optimisation_follows_the_fp32_oracle(dev, precision, sphere_run):
    """The loop of the pose-estimation demo (demo_est_rel_pose.py:74-98) on six numbers: frozen networks (the pair trained on
    the analytic sphere scene: a loss surface with a basin), a camera pose exp(w^) R0 | t0 + dt with learnable (w, dt),
    get_rays -> render_rays -> mse against the image of the true pose -> Adam, 15 steps.

    (a) At every iterate of the fp32 CPU oracle's loop, on the SAME ray values (the oracle's get_rays of that pose) and the
        run's own fine depths (module docstring): dL/d(rays) carried down to the six numbers equals fp32 autograd on the
        oracle: median <= 1e-4 (measured ~1e-6), cosine >= 0.9999, worst case within 3x the fp64 oracle's worst case.
    (b), (c) need a yardstick: the fp64 oracle run beside the fp32 one.  The trained field is sharp: through the 2^9 of the
        positional encoding a one-ulp difference in a ray (the GPU's get_rays against the CPU's) moves the gradient of the six
        numbers by ~1e-3, and end to end it moves a third of the fine depths, some by a whole bin (sample_pdf) -- fp64
        autograd of the oracle sits 1e-3 ... 2e-1 from its own fp32 autograd here.  "Equal to fp32 autograd" can then only mean
        "as close to it as exact arithmetic is": within 3x the fp64 oracle's own distance (floor 1e-3), for
        (b) the end-to-end gradient through the whole GPU path (utils.get_rays on the device included): median and worst
            case over the iterates;
        (c) the free-running loop's distance from the fp32 oracle's, against the free-running fp64 oracle's.
    The bf16 leg prints the same table ("a gradient 23 degrees off fp32" -- here cosine 0.2 and below at some
    iterates even on identical rays and depths) and only has to reduce the loss."""
    from nerf_shared_amd import nerf, render_utils, utils
    H = W = 14
    K = synth.lego_intrinsics(H, W)
    cfg = dict(BASE, N_samples=32, N_importance=48)
    r = render_utils.Renderer(**cfg)
    pairs = []
    for trained in sphere_run[1][:2]:
        sd = {k: v.detach().cpu().clone() for k, v in trained.state_dict().items()}
        m = nerf.NeRF(**VD)
        m.load_state_dict(sd)
        m = m.to(dev)
        m.precision = precision
        m.requires_grad_(False)
        pairs.append((m, {k: v.detach() for k, v in O.state_dict_to_torch(sd).items()}))
    (mc, co), (mf, fo) = pairs
    arch = O.Arch(**VD)
    c2w0 = torch.from_numpy(synth.LEGO_C2W.astype(np.float32))
    ocfg = O.RenderCfg(**cfg)
    w0, dt0 = [0.02, -0.03, 0.015], [0.06, -0.05, 0.04]
    steps, lr = 15, 2e-3

    def assemble(ro, rd):                          # Renderer.render's batch assembly (render_utils.py:205-226)
        ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
        vdir = rd / torch.norm(rd, dim=-1, keepdim=True)
        return torch.cat([ro, rd, 2.0 * torch.ones_like(rd[:, :1]), 6.0 * torch.ones_like(rd[:, :1]), vdir], -1)

    with torch.no_grad():
        target = O.render_rays(ocfg, assemble(*O.get_rays(H, W, K, c2w0)), (co, arch), (fo, arch))["rgb_map"]

    last = {}

    def gpu_loss(pose):
        out = r.render_rays(assemble(*utils.get_rays(H, W, K, pose)), mc, mf, retweights=True)
        last["z"] = out["z_vals"].detach().cpu()
        return utils.img2mse(out["rgb_map"], target.to(dev))

    def cpu_loss(dtype, staged):
        cast = lambda sd: {k: v.to(dtype) for k, v in sd.items()}     # noqa: E731
        c, f = (cast(co), arch), (cast(fo), arch)

        def loss(pose):
            b = assemble(*O.get_rays(H, W, K, pose.to(dtype))).to(dtype)
            rgb = oracle_two_pass(cfg, b, c, f, last["z"].to(dtype))[0] if staged else O.render_rays(ocfg, b, c, f)["rgb_map"]
            return ((rgb - target.to(dtype)) ** 2).mean()
        return loss

    def run(device, loss_fn, forced=None, dtype=torch.float32, also=()):
        """The Adam loop; with forced = a recorded trajectory the gradient is evaluated at ITS iterates (no steps taken), and
        every function of `also` is differentiated at the same iterate right after loss_fn."""
        w = torch.tensor(w0, device=device, dtype=dtype, requires_grad=True)
        dt = torch.tensor(dt0, device=device, dtype=dtype, requires_grad=True)
        opt = torch.optim.Adam([w, dt], lr=lr)
        traj, losses, grads = [], [], [[] for _ in range(1 + len(also))]
        for k in range(steps):
            if forced is not None:
                with torch.no_grad():
                    w.copy_(torch.from_numpy(forced[k][:3]))
                    dt.copy_(torch.from_numpy(forced[k][3:]))
            traj.append(torch.cat([w.detach(), dt.detach()]).cpu().double().numpy().copy())
            for i, fn in enumerate((loss_fn,) + tuple(also)):
                opt.zero_grad()
                if i == 0:
                    loss = fn(_pose(w, dt, c2w0.to(device=device, dtype=dtype)))
                    loss.backward()
                    losses.append(float(loss.detach()))
                else:                                            # a CPU function beside a GPU loop
                    wc, dc = w.detach().cpu().clone().requires_grad_(True), dt.detach().cpu().clone().requires_grad_(True)
                    fn(_pose(wc, dc, c2w0)).backward()
                grads[i].append((torch.cat([w.grad, dt.grad]) if i == 0 else torch.cat([wc.grad, dc.grad])).cpu().double().numpy().copy())
            if forced is None:
                opt.step()
        return np.array(traj), losses, [np.array(g) for g in grads]

    def rel_rows(a, b):
        return np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)

    def cos_rows(a, b):
        return (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))

    cpu = torch.device("cpu")
    # the oracle's own loops do not depend on the leg: run them once per module (the trained pair is the module's too)
    if "oracle" not in _POSE_CACHE:
        ref_, ref_losses_, (g32_,) = run(cpu, cpu_loss(torch.float32, False))
        _, _, (g64_,) = run(cpu, cpu_loss(torch.float64, False), forced=ref_, dtype=torch.float64)
        ref64_, losses64_, _ = run(cpu, cpu_loss(torch.float64, False), dtype=torch.float64)
        _POSE_CACHE["oracle"] = (ref_, ref_losses_, g32_, g64_, ref64_, losses64_)
    ref, ref_losses, g32, g64, ref64, losses64 = _POSE_CACHE["oracle"]
    _, forced_losses, (g_gpu,) = run(dev, gpu_loss, forced=ref)
    # (a) the same ray values on both sides, the oracle's fine pass on the run's depths
    g_same, g32_staged, g64_staged = [], [], []
    co64, fo64 = ({k: v.double() for k, v in co.items()}, arch), ({k: v.double() for k, v in fo.items()}, arch)
    for k in range(steps):
        w = torch.from_numpy(ref[k][:3]).float().requires_grad_(True)
        dt = torch.from_numpy(ref[k][3:]).float().requires_grad_(True)
        ro, rd = O.get_rays(H, W, K, _pose(w, dt, c2w0))
        ro_g, rd_g = ro.detach().to(dev).requires_grad_(True), rd.detach().to(dev).requires_grad_(True)
        out = r.render_rays(assemble(ro_g, rd_g), mc, mf, retweights=True)
        utils.img2mse(out["rgb_map"], target.to(dev)).backward()
        g_same.append(torch.cat(torch.autograd.grad([ro, rd], [w, dt], [ro_g.grad.cpu(), rd_g.grad.cpu()], retain_graph=True)).double().numpy())
        rgb = oracle_two_pass(cfg, assemble(ro, rd), (co, arch), (fo, arch), out["z_vals"].detach().cpu())[0]
        g32_staged.append(torch.cat(torch.autograd.grad(((rgb - target) ** 2).mean(), [w, dt], retain_graph=True)).double().numpy())
        rgb = oracle_two_pass(cfg, assemble(ro, rd).double(), co64, fo64, out["z_vals"].detach().cpu().double())[0]
        g64_staged.append(torch.cat(torch.autograd.grad(((rgb - target.double()) ** 2).mean(), [w, dt])).double().numpy())
    g_same, g32_staged, g64_staged = np.array(g_same), np.array(g32_staged), np.array(g64_staged)
    staged, yard_staged = rel_rows(g_same, g32_staged), rel_rows(g64_staged, g32_staged)
    e2e, yard = rel_rows(g_gpu, g32), rel_rows(g64, g32)
    print(precision, "gradient at the fp32 oracle's iterates, relative L2 from ITS gradient")
    print("  (a) same rays, the run's depths:", ["%.1e" % v for v in staged], "cos min %.8f" % cos_rows(g_same, g32_staged).min())
    print("      the fp64 oracle there:      ", ["%.1e" % v for v in yard_staged], "cos min %.8f" % cos_rows(g64_staged, g32_staged).min())
    print("  (b) end to end:                 ", ["%.1e" % v for v in e2e], "cos min %.6f" % cos_rows(g_gpu, g32).min())
    print("      the fp64 oracle:            ", ["%.1e" % v for v in yard], "cos min %.6f" % cos_rows(g64, g32).min())
    print("  loss there", ["%.6f" % v for v in forced_losses[::2]], "fp32 oracle", ["%.6f" % v for v in ref_losses[::2]])
    got, losses, _ = run(dev, gpu_loss)
    travelled = np.abs(ref[-1] - np.array(w0 + dt0)).max()
    drift, drift64 = np.abs(got - ref).max(axis=1), np.abs(ref64 - ref).max(axis=1)
    print("free-running loop: loss", ["%.5f" % v for v in losses[::2]])
    print("      fp32 oracle: loss", ["%.5f" % v for v in ref_losses[::2]])
    print("      fp64 oracle: loss", ["%.5f" % v for v in losses64[::2]])
    print("  max |parameter - fp32 oracle's| per step", ["%.1e" % v for v in drift])
    print("  the fp64 oracle's                       ", ["%.1e" % v for v in drift64], "; the fp32 oracle travelled %.3e" % travelled)
    assert losses[-1] < 0.6 * losses[0] and ref_losses[-1] < 0.6 * ref_losses[0]
    if precision == "fp32_split":
        np.testing.assert_allclose(forced_losses, ref_losses, rtol=1e-2)
        # (a): ~1e-6 except where a ReLU sits within rounding of zero at a point that carries the image's gradient (the fp64
        # oracle shows the same sporadic 1e-3 ... 1e-2 against the fp32 one): typical value and direction gated tightly, the
        # worst case against the fp64 oracle's worst case
        assert np.median(staged) < 1e-4 and cos_rows(g_same, g32_staged).min() > GATE_COS, staged
        assert staged.max() < 3.0 * max(yard_staged.max(), 1e-3), (staged, yard_staged)
        # (b), (c): against the fp64 oracle's own distance from the fp32 oracle (the kinks are hit at different iterates by
        # different arithmetics, so typical and worst values are compared, not iterate by iterate)
        assert np.median(e2e) < 3.0 * max(np.median(yard), 1e-3) and e2e.max() < 3.0 * max(yard.max(), 1e-3), (e2e, yard)
        assert drift.max() < 3.0 * max(drift64.max(), 1e-3 * travelled), (drift, drift64)


def test_loss_scale_is_invisible(dev):
    """dL/draw enters the chain multiplied by a power of two taken from its own maximum (csrc/split.h): gradients of a loss
    scaled by 2^-20 and by 2^+12 are the same gradients scaled (exactly: powers of two), and a zero gradient gives zeros."""
    rng = np.random.default_rng(3)
    pts = torch.from_numpy(rng.uniform(-2, 2, size=(33, 7, 3)).astype(np.float32)).to(dev)
    vd = torch.from_numpy(rng.normal(size=(33, 3)).astype(np.float32)).to(dev)
    coef = torch.from_numpy(rng.normal(size=(33, 7, 4)).astype(np.float32)).to(dev)
    m, _ = models(dev, 1, 2.0, VD, "fp32_split")
    grads = {}
    for k in (0.0, 1.0, 2.0 ** -20, 2.0 ** 12):
        m.zero_grad()
        (m(pts, vd) * coef).sum().mul(k).backward()
        grads[k] = {n: p.grad.clone() for n, p in m.named_parameters()}
    for n in grads[1.0]:
        assert torch.isfinite(grads[1.0][n]).all()
        assert not grads[0.0][n].any(), n
        assert torch.equal(grads[2.0 ** -20][n], grads[1.0][n] * 2.0 ** -20), n
        assert torch.equal(grads[2.0 ** 12][n], grads[1.0][n] * 2.0 ** 12), n


def test_frozen_model_keeps_its_own_precision_in_a_training_call(dev):
    """A frozen fine model beside a training coarse model: the fine pass runs on the forward-only kernel of ITS precision (it
    used to be dragged through the bf16 training forward) and only the coarse model gets gradients."""
    from nerf_shared_amd import render_utils
    batch, target = _batch(64, 9)
    cfg = dict(BASE, N_samples=32, N_importance=32)
    r = render_utils.Renderer(**cfg)
    mc, _ = models(dev, 1, 2.0, VD, "bf16")
    mf, _ = models(dev, 11, 2.0, VD, "fp32")
    mf.requires_grad_(False)
    out = r.render_rays(batch.to(dev), mc, mf, retraw=True, retweights=True)
    assert out["rgb0"].requires_grad and not out["rgb_map"].requires_grad
    with torch.no_grad():
        pts = batch[:, None, 0:3].to(dev) + batch[:, None, 3:6].to(dev) * out["z_vals"][:, :, None]
        want = mf(pts, batch[:, 8:11].to(dev))
    assert torch.equal(out["raw"], want)                                   # the exact-fp32 kernel's values, not bf16's
    (((out["rgb_map"] - target.to(dev)) ** 2).mean() + ((out["rgb0"] - target.to(dev)) ** 2).mean()).backward()
    assert all(p.grad is not None for p in mc.parameters()) and all(p.grad is None for p in mf.parameters())


@pytest.mark.parametrize("variant", ["single_model_both_passes", "coarse_only", "noise_lindisp_perturb", "ndc_fern"])
def test_training_gradients_of_the_other_render_configurations_match_fp32_autograd(dev, variant):
    """render_rays' other branches under autograd in split precision: fine_model=None (the coarse network evaluates both
    passes, render_utils.py:150-151: its gradient is the sum of two backward passes), N_importance=0, lindisp + stratified
    jitter + sigma noise (seeded draws on both sides), and the LLFF configuration (configs/fern.txt: NDC rays, near/far 0/1,
    64+64-style sampling, noise, black background) -- against fp32 autograd on the oracle."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from nerf_shared_amd import render_utils
    from test_gpu_parity import oracle_batch
    batch, target = _batch(64, 5)
    cfg = dict(BASE, N_samples=32, N_importance=0 if variant == "coarse_only" else 40)
    use_pytest = variant in ("noise_lindisp_perturb", "ndc_fern")
    if variant == "noise_lindisp_perturb":
        cfg.update(lindisp=True, raw_noise_std=1.0, perturb=1.0)
    if variant == "ndc_fern":
        H, W, focal = 378, 504, 408.0
        K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
        c2w = np.array([[1, 0, 0, 0.05], [0, 1, 0, -0.02], [0, 0, 1, 0.1]], np.float32)
        cfg.update(ndc=True, near=0.0, far=1.0, white_bkgd=False, raw_noise_std=1.0, perturb=1.0, N_importance=32)
        batch = oracle_batch(cfg, H, W, K, c2w, np.sort(np.random.default_rng(12).choice(H * W, size=64, replace=False)))
    r = render_utils.Renderer(**cfg)
    mc, cc = models(dev, 1, 1.0, VD, "fp32_split")
    mf, cf = models(dev, 11, 1.0, VD, "fp32_split")
    with torch.no_grad():            # lift the density bias: a semi-transparent volume, non-degenerate gradients
        for m, sd in ((mc, cc), (mf, cf)):
            m.alpha_linear.bias += 0.3
            sd["alpha_linear.bias"] += 0.3
    use_fine = variant in ("noise_lindisp_perturb", "ndc_fern")
    out = r.render_rays(batch.to(dev), mc, mf if use_fine else None, retweights=True, pytest=use_pytest)
    t = target.to(dev)
    loss = ((out["rgb_map"] - t) ** 2).mean()
    if "rgb0" in out:
        loss = loss + ((out["rgb0"] - t) ** 2).mean()
    loss.backward()
    assert use_fine or all(p.grad is None for p in mf.parameters())
    oc, of = (cc, O.Arch(**VD)), ((cf, O.Arch(**VD)) if use_fine else (cc, O.Arch(**VD)))
    if variant == "coarse_only":
        o = O.render_rays(O.RenderCfg(**cfg), batch, oc, None)
        l = ((o["rgb_map"] - target) ** 2).mean()
    else:
        rgb, rgb0 = oracle_two_pass(cfg, batch, oc, of, out["z_vals"].detach().cpu(), pytest_draws=use_pytest)
        l = ((rgb - target) ** 2).mean() + ((rgb0 - target) ** 2).mean()
    l.backward()
    assert abs(float(loss) - float(l)) < 5e-6 * max(1.0, abs(float(l))), (float(loss), float(l))
    table = []
    check_params("coarse.", mc, cc, table)
    if use_fine:
        check_params("fine.", mf, cf, table)
    assert all(float(cc[n].grad.norm()) > 0 for n in cc if cc[n].grad is not None), "degenerate test: zero gradient"
    assert_table(table)


def smallest_preactivation(cpu, arch, pts, vd):
    """min |pre-activation| over the hidden ReLU units of NeRF.MLP (nerf.py:110-134) on the fp32 oracle: a unit within fp32
    rounding of zero may sit on the other side in any other fp32-class evaluation (fp64 included), and then its whole
    gradient column differs -- one flip among n points moves a tensor's gradient by ~sqrt(1 / (128 n))."""
    with torch.no_grad():
        sd = {k: v.detach() for k, v in cpu.items()}
        e = O.embed(pts.reshape(-1, 3), arch["multires"])
        h, small = e, float("inf")
        for i in range(8):
            a = torch.nn.functional.linear(h, sd["pts_linears.%d.weight" % i], sd["pts_linears.%d.bias" % i])
            small = min(small, float(a.abs().min()))
            h = torch.relu(a)
            if i == 4:
                h = torch.cat([e, h], -1)
        feat = torch.nn.functional.linear(h, sd["feature_linear.weight"], sd["feature_linear.bias"])
        d = O.embed(vd[:, None].expand(pts.shape).reshape(-1, 3), arch["multires_views"])
        a = torch.nn.functional.linear(torch.cat([feat, d], -1), sd["views_linears.0.weight"], sd["views_linears.0.bias"])
        return min(small, float(a.abs().min()))


@pytest.mark.parametrize("n_points", [1, 15, 16, 17, 127, 128, 129, 255, 257, 2049])
def test_field_backward_on_awkward_point_counts(dev, n_points):
    """Point counts around the kernels' tiles (16 points per wave, 128 per workgroup, 32 per weight-gradient chunk, 256-row
    padding of the training arrays): the padding points must contribute nothing.  With so few points ONE ReLU unit on the
    other side of zero is visible (3e-3 at 257 points), so the draw is repeated until the oracle has no unit within 1e-5 of
    zero -- what is tested here is the padding, not the conditioning of ReLU."""
    m, cpu = models(dev, 1, 2.0, VD, "fp32_split")
    for attempt in range(20):
        rng = np.random.default_rng(100 + n_points + 1000 * attempt)
        pts = torch.from_numpy(rng.uniform(-2, 2, size=(n_points, 1, 3)).astype(np.float32))
        vd = torch.from_numpy(rng.normal(size=(n_points, 3)).astype(np.float32))
        coef = torch.from_numpy(rng.normal(size=(n_points, 1, 4)).astype(np.float32))
        if smallest_preactivation(cpu, VD, pts, vd) > 1e-5:
            break
    (O.nerf_forward(cpu, O.Arch(**VD), pts, vd) * coef).sum().backward()
    (m(pts.to(dev), vd.to(dev)) * coef.to(dev)).sum().backward()
    table = []
    check_params("", m, cpu, table)
    assert_table(table)


def scaled_models(dev, seed, arch, precision, k):
    """models() with the first layer's weight and bias times k: every hidden unit of layer 0 (and its ReLU output) scales
    by k exactly."""
    from nerf_shared_amd import nerf
    sd = synth.torch_state_dict(seed, 1.0, **{**arch, "skips": (4,)})
    for name in ("pts_linears.0.weight", "pts_linears.0.bias"):
        sd[name] = sd[name] * k
    m = nerf.NeRF(**arch)
    m.load_state_dict(sd)
    m = m.to(dev)
    m.precision = precision
    cpu = {k_: v.clone().requires_grad_(True) for k_, v in O.state_dict_to_torch(sd).items()}
    return m, cpu


@pytest.mark.parametrize("arch", [VD, NOVD], ids=["viewdirs", "output_linear"])
def test_fp32_trains_beyond_the_fp16_range(dev, arch):
    """The case 'fp32' exists for (set_default_precision): a fused-family model whose first hidden layer, after its ReLU,
    reaches 1e5 on the oracle -- beyond fp16's 65504, so the split kernels' hi parts overflow.  In 'fp32' the training
    forward passes the fp32 forward gate (rel-L2 1e-5 against the oracle) and the parameter, point and view-direction
    gradients are finite and within 2e-5 of fp32 autograd; the same model in 'fp32_split' fails that forward gate (non-finite
    output counts as failing), which keeps the documented limit honest and shows the case really is out of fp16's range."""
    vdirs = bool(arch["use_viewdirs"])
    rng = np.random.default_rng(31)
    R, S = 60, 11
    pts = torch.from_numpy(rng.uniform(-2, 2, size=(R, S, 3)).astype(np.float32))
    vd = torch.from_numpy(rng.normal(size=(R, 3)).astype(np.float32)) if vdirs else None
    out_ch = 4 if vdirs else arch["output_ch"]
    coef = torch.from_numpy(rng.normal(size=(R, S, out_ch)).astype(np.float32))
    m, cpu = scaled_models(dev, 6, arch, "fp32", 1e5)
    with torch.no_grad():
        h0 = torch.relu(O._lin(cpu, "pts_linears.0", O.embed(pts.reshape(-1, 3), arch["multires"])))
    print("largest post-ReLU activation of layer 0 on the oracle: %.3e" % float(h0.max()))
    assert float(h0.max()) > 1e5, "degenerate test: the model is inside fp16's range"
    p_cpu = pts.clone().requires_grad_(True)
    v_cpu = vd.clone().requires_grad_(True) if vdirs else None
    ref = O.nerf_forward(cpu, O.Arch(**arch), p_cpu, v_cpu)
    (ref * coef).sum().backward()
    p_gpu = pts.to(dev).requires_grad_(True)
    v_gpu = vd.to(dev).requires_grad_(True) if vdirs else None
    out = m(p_gpu, v_gpu)
    (out * coef.to(dev)).sum().backward()
    e_fwd = rel_err(out.detach().cpu(), ref.detach())
    table = [("pts", rel_err(p_gpu.grad.cpu(), p_cpu.grad), cosine(p_gpu.grad, p_cpu.grad))]
    assert torch.isfinite(p_gpu.grad).all()
    if vdirs:
        assert torch.isfinite(v_gpu.grad).all()
        table.append(("viewdirs", rel_err(v_gpu.grad.cpu(), v_cpu.grad), cosine(v_gpu.grad, v_cpu.grad)))
    check_params("", m, cpu, table)
    print("'fp32' forward rel-L2 vs the oracle %.3e" % e_fwd)
    assert e_fwd <= 1e-5
    assert_table(table, gate_rel=2e-5)
    # the same model in split precision: out of its range
    ms, _ = scaled_models(dev, 6, arch, "fp32_split", 1e5)
    out_s = ms(pts.to(dev).requires_grad_(True), vd.to(dev) if vdirs else None).detach().cpu()
    finite = bool(torch.isfinite(out_s).all())
    e_split = rel_err(out_s, ref.detach()) if finite else float("inf")
    print("'fp32_split' forward: finite %s, rel-L2 vs the oracle %.3e" % (finite, e_split))
    assert not (finite and e_split <= 1e-5), "fp32_split passed the fp32 gate beyond fp16's range"


def test_split_training_point_limit_is_refused_before_the_workspace_check(dev):
    """nerf_amd_field_forward_train / nerf_amd_field_backward in NERF_AMD_PREC_FP32_SPLIT refuse more than
    NERF_AMD_SPLIT_TRAIN_MAX_POINTS = 2^23 - 256 points (the weight-gradient kernel's 32-bit buffer offsets would wrap), before
    they look at the workspace: with a 1-byte workspace the limit itself fails on 'workspace too small', one point more on
    the limit.  Nothing of that size is allocated and no kernel runs (both calls return before any launch)."""
    import ctypes
    import re

    from nerf_shared_amd import _lib, nerf
    lim = nerf._SPLIT_TRAIN_MAX_POINTS
    assert lim == (1 << 23) - 256
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerf_amd.h")) as f:
        assert int(re.search(r"#define NERF_AMD_SPLIT_TRAIN_MAX_POINTS\s+(\d+)", f.read()).group(1)) == lim
    m, _ = models(dev, 0, 1.0, VD, "fp32_split")
    h = m._model_handle(dev, _lib.TRAIN_COPIES[_lib.PREC_FP32_SPLIT] | _lib.TRAIN_COPIES[_lib.PREC_BF16])
    buf = torch.zeros(64, device=dev)             # stands in for every array: no call below reads or writes it
    ws = torch.empty(1, dtype=torch.uint8, device=dev)
    n = len(m._grad_layout()[1])
    gw = (ctypes.c_void_p * n)(*[buf.data_ptr()] * n)
    gb = (ctypes.c_void_p * n)(*[buf.data_ptr()] * n)
    stream = _lib.stream_of(dev)

    def calls(P, prec):
        b = buf.data_ptr()
        fwd = _lib.lib.nerf_amd_field_forward_train(h, b, b, None, 0, None, P, 1, b, ws.data_ptr(), ws.numel(), prec, stream)
        fwd_msg = _lib.lib.nerf_amd_last_error().decode()
        bwd = _lib.lib.nerf_amd_field_backward(h, b, b, b, None, 0, None, P, 1, ws.data_ptr(), ws.numel(), gw, gb, n,
                                               None, None, None, prec, stream)
        bwd_msg = _lib.lib.nerf_amd_last_error().decode()
        return (fwd, fwd_msg), (bwd, bwd_msg)

    for rc, msg in calls(lim, _lib.PREC_FP32_SPLIT):
        assert rc == -1 and "workspace too small" in msg, msg
    for rc, msg in calls(lim + 1, _lib.PREC_FP32_SPLIT):
        assert rc == -1 and "NERF_AMD_SPLIT_TRAIN_MAX_POINTS = %d" % lim in msg and "workspace" not in msg, msg
    for rc, msg in calls(lim + 1, _lib.PREC_BF16):                 # the bf16 kernels address with 64 bits: no such limit
        assert rc == -1 and "workspace too small" in msg, msg
    torch.cuda.synchronize()


def _split_field_run(dev, arch, pts, vd, coef):
    m, cpu = models(dev, 3, 2.0, arch, "fp32_split")
    p_gpu = pts.to(dev).requires_grad_(True)
    v_gpu = vd.to(dev).requires_grad_(True) if vd is not None else None
    out = m(p_gpu, v_gpu)
    (out * coef.to(dev)).sum().backward()
    grads = {name: p.grad.detach().clone() for name, p in m.named_parameters() if p.grad is not None}
    grads["pts"] = p_gpu.grad.detach().clone()
    if v_gpu is not None:
        grads["viewdirs"] = v_gpu.grad.detach().clone()
    return out.detach(), grads, m, cpu


@pytest.mark.parametrize("arch", [VD, NOVD], ids=["viewdirs", "output_linear"])
def test_split_training_above_the_point_limit_runs_in_pieces_of_whole_rays(dev, arch, monkeypatch):
    """NeRF.forward in 'fp32_split' with more points than nerf._SPLIT_TRAIN_MAX_POINTS (lowered here to 300, so that 70 rays of
    13 samples go in pieces of 23 rays, the last one ragged): raw bit-identical to the call in one piece, parameter / point /
    view-direction gradients within the split gates of fp32 autograd on the oracle and within 1e-5 of the one-piece run
    (each piece takes its own loss scale, so they are not bit-identical)."""
    from nerf_shared_amd import nerf
    rng = np.random.default_rng(11)
    R, S = 70, 13
    pts = torch.from_numpy(rng.uniform(-2, 2, size=(R, S, 3)).astype(np.float32))
    vd = torch.from_numpy(rng.normal(size=(R, 3)).astype(np.float32))
    vd = vd / vd.norm(dim=-1, keepdim=True)
    if not arch["use_viewdirs"]:
        vd = None
    coef = torch.from_numpy(rng.normal(size=(R, S, 4 if arch["use_viewdirs"] else arch["output_ch"])).astype(np.float32))
    raw1, g1, _, _ = _split_field_run(dev, arch, pts, vd, coef)
    monkeypatch.setattr(nerf, "_SPLIT_TRAIN_MAX_POINTS", 300)
    calls = []
    real_apply = nerf._FieldTrainFn.apply
    monkeypatch.setattr(nerf._FieldTrainFn, "apply", lambda *a: calls.append(a[6] * a[7]) or real_apply(*a))
    raw2, g2, m, cpu = _split_field_run(dev, arch, pts, vd, coef)
    assert calls == [299, 299, 299, 13], calls
    assert torch.equal(raw2, raw1)
    p_cpu = pts.clone().requires_grad_(True)
    v_cpu = vd.clone().requires_grad_(True) if vd is not None else None
    (O.nerf_forward(cpu, O.Arch(**arch), p_cpu, v_cpu) * coef).sum().backward()
    table = [("pts", rel_err(g2["pts"], p_cpu.grad), cosine(g2["pts"], p_cpu.grad))]
    if vd is not None:
        table.append(("viewdirs", rel_err(g2["viewdirs"], v_cpu.grad), cosine(g2["viewdirs"], v_cpu.grad)))
    check_params("", m, cpu, table)
    assert_table(table)
    for name in g1:
        e = rel_err(g2[name], g1[name])
        assert e < 1e-5, (name, e)


def test_split_training_step_above_the_point_limit_runs_in_pieces_of_whole_rays(dev, monkeypatch):
    """The two-pass training loss of Renderer.render_rays (rays mode: pts = o + d z in the kernel) in 'fp32_split' with the
    point limit lowered to 500 (coarse pass: pieces of 15 rays x 32 samples, fine pass: 6 rays x 80; 80 rays): raw and depths
    bit-identical to the run in one piece; parameter and ray gradients within the split gates of fp32 autograd on the oracle
    (fine pass on the run's own depths) and within 1e-5 of the one-piece run."""
    from nerf_shared_amd import nerf, render_utils
    batch, target = _batch(80, 7)                   # test_ray_gradients_for_pose_estimation_match_fp32_autograd's rays
    cfg = dict(BASE, N_samples=32, N_importance=48)
    r = render_utils.Renderer(**cfg)

    def assemble(o, d):
        return torch.cat([o, d, 2.0 * torch.ones_like(d[:, :1]), 6.0 * torch.ones_like(d[:, :1]),
                          d / torch.norm(d, dim=-1, keepdim=True)], -1)

    def run():
        mc, cc = models(dev, 1, 2.0, VD, "fp32_split")
        mf, cf = models(dev, 11, 2.0, VD, "fp32_split")
        ro = batch[:, 0:3].clone().to(dev).requires_grad_(True)
        rd = (batch[:, 3:6] * 1.3).clone().to(dev).requires_grad_(True)
        out = r.render_rays(assemble(ro, rd), mc, mf, retraw=True, retweights=True)
        t = target.to(dev)
        (((out["rgb_map"] - t) ** 2).mean() + ((out["rgb0"] - t) ** 2).mean()).backward()
        grads = {"coarse." + k: p.grad.detach().clone() for k, p in mc.named_parameters() if p.grad is not None}
        grads.update({"fine." + k: p.grad.detach().clone() for k, p in mf.named_parameters() if p.grad is not None})
        grads.update(rays_o=ro.grad.detach().clone(), rays_d=rd.grad.detach().clone())
        return out, grads, (mc, cc), (mf, cf)

    out1, g1, _, _ = run()
    monkeypatch.setattr(nerf, "_SPLIT_TRAIN_MAX_POINTS", 500)
    out2, g2, (mc, cc), (mf, cf) = run()
    assert torch.equal(out2["raw"], out1["raw"]) and torch.equal(out2["z_vals"], out1["z_vals"])
    o = batch[:, 0:3].clone().requires_grad_(True)
    d = (batch[:, 3:6] * 1.3).clone().requires_grad_(True)
    rgb, rgb0 = oracle_two_pass(cfg, assemble(o, d), (cc, O.Arch(**VD)), (cf, O.Arch(**VD)), out2["z_vals"].detach().cpu())
    (((rgb - target) ** 2).mean() + ((rgb0 - target) ** 2).mean()).backward()
    table = [("rays_o", rel_err(g2["rays_o"], o.grad), cosine(g2["rays_o"], o.grad)),
             ("rays_d", rel_err(g2["rays_d"], d.grad), cosine(g2["rays_d"], d.grad))]
    check_params("coarse.", mc, cc, table)
    check_params("fine.", mf, cf, table)
    assert_table(table)
    for name in g1:
        e = rel_err(g2[name], g1[name])
        assert e < 1e-5, (name, e)
