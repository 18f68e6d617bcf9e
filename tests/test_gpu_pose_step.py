"""GPU tests (-m gpu) of the pose-estimation workload (demo_est_rel_pose.py:74-98) on the device: rays at selected pixels with
the pose read from device memory (utils.get_rays_at), the demo's se(3) module as one kernel each way (utils.CameraTransf),
the inputs-only field backward (nerf_amd_field_backward_inputs behind frozen models) and the captured loop body
(utils.CapturedPoseStep).

Every bound is either exact (torch.equal), derived from the number formats, or a multiple of a yardstick measured in the
same test (fp32 torch against fp64 torch; one eager run against another), never a number taken from the code under test."""
import ctypes
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
pytestmark = pytest.mark.gpu

from nerf_shared_amd import _lib, synth  # noqa: E402
from test_gpu_backward import BASE, VD, _batch, rel_err  # noqa: E402

SIZES = [1, 63, 64, 65, 257, 1000]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def lego44():
    return np.concatenate([synth.LEGO_C2W, np.array([[0, 0, 0, 1]], np.float32)], 0)


_DENSE = {}


def dense_rays(H, W, c2w_np, dev):
    """utils.get_rays over the whole image, once per (H, W, pose): the reference of every selection test."""
    from nerf_shared_amd import utils
    key = (H, W, c2w_np.tobytes())
    if key not in _DENSE:
        _DENSE[key] = utils.get_rays(H, W, synth.lego_intrinsics(H, W), torch.from_numpy(c2w_np[:3].copy()).to(dev))
    return _DENSE[key]


def pixel_cases():
    """(id, H, W, pixels [n, 2] int64 numpy (x, y))."""
    rng = np.random.default_rng(3)
    cases = []
    all35 = np.stack(np.meshgrid(np.arange(7), np.arange(5), indexing="xy"), -1).reshape(-1, 2)
    shuffled = all35[rng.permutation(35)]
    cases.append(("5x7_all_shuffled_plus_duplicates", 5, 7, np.concatenate([shuffled, shuffled[[3, 3, 17, 0, 34, 34]]], 0)))
    cases.append(("800_corners", 800, 800, np.array([[0, 0], [799, 0], [0, 799], [799, 799], [799, 0]])))
    for n in SIZES:
        cases.append(("800_n%d" % n, 800, 800, np.stack([rng.integers(0, 800, size=n), rng.integers(0, 800, size=n)], -1)))
    return cases


CASES = pixel_cases()


# ------------------------------------------------------------------------------------------------ 1. rays, forward
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("rows", [3, 4], ids=["c2w_3x4", "c2w_4x4"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
def test_rays_at_pixels_equal_get_rays_bit_for_bit(dev, case, rows, dtype):
    """get_rays_at(H, W, K, c2w, pixels) == get_rays(H, W, K, c2w)[y, x], torch.equal, for rays_o and rays_d."""
    from nerf_shared_amd import utils
    _, H, W, pix = case
    pose = lego44()
    o_ref, d_ref = dense_rays(H, W, pose, dev)
    c2w = torch.from_numpy(pose[:rows].copy()).to(dev)
    p = torch.from_numpy(pix).to(device=dev, dtype=dtype)
    o, d = utils.get_rays_at(H, W, synth.lego_intrinsics(H, W), c2w, p)
    assert o.shape == d.shape == (pix.shape[0], 3) and o.dtype == d.dtype == torch.float32
    y, x = torch.from_numpy(pix[:, 1]).to(dev), torch.from_numpy(pix[:, 0]).to(dev)
    assert torch.equal(o, o_ref[y, x])
    assert torch.equal(d, d_ref[y, x])


def test_rays_at_pixels_take_host_pixels_and_a_row_strided_pose(dev):
    """A list of pixels (checked on the host) and the top of a [4, 4] that is itself a view with a row stride of 8."""
    from nerf_shared_amd import utils
    H, W = 5, 7
    wide = torch.zeros(4, 8, device=dev)
    wide[:, :4] = torch.from_numpy(lego44()).to(dev)
    o_ref, d_ref = dense_rays(H, W, lego44(), dev)
    o, d = utils.get_rays_at(H, W, synth.lego_intrinsics(H, W), wide[:, :4], [[6, 4], [0, 0], [3, 2]])
    assert torch.equal(o, o_ref[[4, 0, 2], [6, 0, 3]]) and torch.equal(d, d_ref[[4, 0, 2], [6, 0, 3]])


# ------------------------------------------------------------------------------------------------ 2. pose on the device
def test_a_captured_get_rays_at_reads_the_pose_at_replay_time(dev):
    """The property get_rays cannot have (it copies the pose to the host): captured once in a HIP graph, the call sees the
    pose tensor's CURRENT contents on every replay."""
    from nerf_shared_amd import utils
    H = W = 40
    K = synth.lego_intrinsics(H, W)
    rng = np.random.default_rng(9)
    pix = torch.from_numpy(np.stack([rng.integers(0, W, size=300), rng.integers(0, H, size=300)], -1)).to(dev)       # int64: converted in the graph
    c2w = torch.from_numpy(lego44()).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        utils.get_rays_at(H, W, K, c2w, pix)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o, d = utils.get_rays_at(H, W, K, c2w, pix)
    graph.replay()
    o_first, d_first = o.clone(), d.clone()
    new_pose = synth.pose_spherical(40.0)
    c2w[:3].copy_(torch.from_numpy(new_pose).to(dev))
    graph.replay()
    eo, ed = utils.get_rays_at(H, W, K, c2w, pix)
    assert torch.equal(o, eo) and torch.equal(d, ed)
    o_ref, d_ref = utils.get_rays(H, W, K, torch.from_numpy(new_pose))
    assert torch.equal(o, o_ref[pix[:, 1], pix[:, 0]]) and torch.equal(d, d_ref[pix[:, 1], pix[:, 0]])
    assert not torch.equal(o, o_first) and not torch.equal(d, d_first)


# ------------------------------------------------------------------------------------------------ 3. rays, backward
def rays_bwd(dev, H, W, pix, g_o, g_d):
    """nerf_amd_rays_at_pixels_backward, called directly (either gradient may be None)."""
    K = synth.lego_intrinsics(H, W)
    k4 = (ctypes.c_double * 4)(float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
    n = pix.shape[0]
    out = torch.full((12,), float("nan"), device=dev)
    partials = torch.empty(256 * 12, device=dev) if n > 16384 else None
    _lib.check(_lib.lib.nerf_amd_rays_at_pixels_backward(H, W, k4, pix.data_ptr(), n, _lib.ptr(g_o), _lib.ptr(g_d), out.data_ptr(),
                                                         _lib.ptr(partials), _lib.stream_of(dev)), "nerf_amd_rays_at_pixels_backward")
    return out.cpu().double().numpy().reshape(3, 4)


def pose_grad_reference(H, W, pix, g_o, g_d):
    """float64 sums on the CPU from the same pixels: (g_c2w [3, 4], sum of |terms| [3, 4])."""
    K = synth.lego_intrinsics(H, W)
    fx, fy, cx, cy = (float(np.float32(v)) for v in (K[0][0], K[1][1], K[0][2], K[1][2]))       # the kernel's fp32 intrinsics
    x, y = pix[:, 0].astype(np.float64), pix[:, 1].astype(np.float64)
    dirs = np.stack([(x - cx) / fx, -(y - cy) / fy, -np.ones_like(x)], -1)
    ref, mag = np.zeros((3, 4)), np.zeros((3, 4))
    if g_d is not None:
        terms = g_d.astype(np.float64)[:, :, None] * dirs[:, None, :]                            # [n, k, m]
        ref[:, :3], mag[:, :3] = terms.sum(0), np.abs(terms).sum(0)
    if g_o is not None:
        ref[:, 3], mag[:, 3] = g_o.astype(np.float64).sum(0), np.abs(g_o.astype(np.float64)).sum(0)
    return ref, mag


_RNG4 = np.random.default_rng(4)
BWD_CASES = CASES + [("800_n20000_two_stage", 800, 800, np.stack([_RNG4.integers(0, 800, size=20000), _RNG4.integers(0, 800, size=20000)], -1))]


@pytest.mark.parametrize("case", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_rays_at_pixels_backward_is_the_float64_sum_and_order_fixed(dev, case):
    """|g_c2w - float64 sum| <= 1e-5 * sum |terms| per entry (a tree sum of <= 1000 fp32 terms errs by about
    log2(n) 2^-24 ~ 6e-7 of that; the margin covers the per-thread serial part and the fp32 pixel directions), with both
    gradients, with g_o = None and with g_d = None; and two calls on the same inputs are torch.equal.  (The 20000-pixel
    case is beyond the one-launch limit of 16384: per-block sums, then the finish kernel.)"""
    _, H, W, pix = case
    rng = np.random.default_rng(pix.shape[0])
    n = pix.shape[0]
    g_o_np, g_d_np = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
    p = torch.from_numpy(pix).to(device=dev, dtype=torch.int32).contiguous()
    g_o, g_d = torch.from_numpy(g_o_np).to(dev), torch.from_numpy(g_d_np).to(dev)
    for tag, (a, b) in {"both": (g_o, g_d), "g_o=None": (None, g_d), "g_d=None": (g_o, None)}.items():
        got = rays_bwd(dev, H, W, p, a, b)
        ref, mag = pose_grad_reference(H, W, pix, None if a is None else g_o_np, None if b is None else g_d_np)
        err = np.abs(got - ref)
        print("%s %s: worst |got - ref| / sum|terms| = %.3e" % (case[0], tag, float((err / np.maximum(mag, 1e-300)).max())))
        assert np.isfinite(got).all() and (err <= 1e-5 * mag).all(), (tag, got, ref)
        again = rays_bwd(dev, H, W, p, a, b)
        assert np.array_equal(got, again), tag


@pytest.mark.parametrize("case", [CASES[0], CASES[6]], ids=[CASES[0][0], CASES[6][0]])
@pytest.mark.parametrize("rows", [3, 4], ids=["c2w_3x4", "c2w_4x4"])
def test_pose_gradient_through_autograd_equals_get_rays_then_index(dev, case, rows):
    """c2w.grad of get_rays_at against c2w.grad of get_rays(...)[y, x] (a dense [H, W, 3] gradient, zero almost everywhere,
    summed with float atomics) for a random linear loss: the same bound, and the float64 sums between them."""
    from nerf_shared_amd import utils
    _, H, W, pix = case
    K = synth.lego_intrinsics(H, W)
    n = pix.shape[0]
    rng = np.random.default_rng(31)
    co_np, cd_np = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
    co, cd = torch.from_numpy(co_np).to(dev), torch.from_numpy(cd_np).to(dev)
    p = torch.from_numpy(pix).to(dev)
    a = torch.from_numpy(lego44()[:rows].copy()).to(dev).requires_grad_(True)
    o, d = utils.get_rays_at(H, W, K, a, p)
    ((o * co).sum() + (d * cd).sum()).backward()
    b = torch.from_numpy(lego44()[:rows].copy()).to(dev).requires_grad_(True)
    o2, d2 = utils.get_rays(H, W, K, b)
    ((o2[p[:, 1], p[:, 0]] * co).sum() + (d2[p[:, 1], p[:, 0]] * cd).sum()).backward()
    assert a.grad.shape == b.grad.shape == (rows, 4)
    # duplicates: the dense path sums their coefficients into one pixel first; the bound is on the sum of |terms| either way
    ref, mag = pose_grad_reference(H, W, pix, co_np, cd_np)
    ga, gb = a.grad.cpu().double().numpy(), b.grad.cpu().double().numpy()
    assert (np.abs(ga[:3] - ref) <= 1e-5 * mag).all() and (np.abs(ga[:3] - gb[:3]) <= 1e-5 * mag).all()
    if rows == 4:
        assert not ga[3].any() and not gb[3].any()


# ------------------------------------------------------------------------------------------------ 4. se(3)
def se3_torch(w, v, theta, x):
    """T = exp_i @ x from the formula (K = [w]x), in the dtype of its arguments."""
    z = torch.zeros((), dtype=w.dtype)
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    I, K2 = torch.eye(3, dtype=w.dtype), K @ K
    s, c = torch.sin(theta), torch.cos(theta)
    R = I + s * K + (1 - c) * K2
    u = (theta * I + (1 - c) * K + (theta - s) * K2) @ v
    bottom = torch.tensor([[0, 0, 0, 1]], dtype=w.dtype)
    return torch.cat([torch.cat([R, u[:, None]], 1), bottom], 0) @ x


def se3_params(which):
    rng = np.random.default_rng(17)
    if which == "init_scale":
        return rng.normal(0, 1e-6, 3), rng.normal(0, 1e-6, 3), rng.normal(0, 1e-6)
    w = rng.normal(size=3)
    v = rng.normal(size=3)
    return w / np.linalg.norm(w) * 1.03, v / np.linalg.norm(v) * 0.5, {"theta_0.3": 0.3, "theta_2.5": 2.5}[which]


@pytest.mark.parametrize("which", ["init_scale", "theta_0.3", "theta_2.5"])
def test_camera_transf_matches_the_formula_in_float64(dev, which):
    """Forward: max abs error against float64 <= 2x the float32 torch evaluation's own error (floor: 4 ulp of the largest
    entry).  Backward with a random g_T: relative L2 against float64 autograd <= 2x float32 autograd's own distance (floor
    1e-6).  x requires grad, gets none, and nothing is raised."""
    from nerf_shared_amd import utils
    w_np, v_np, th_np = (np.asarray(a, dtype=np.float32) for a in se3_params(which))
    x_np = lego44()
    g_np = np.random.default_rng(23).normal(size=(4, 4)).astype(np.float32)

    def cpu(dtype):
        w, v, th = (torch.from_numpy(a.copy()).to(dtype).requires_grad_(True) for a in (w_np, v_np, th_np))
        T = se3_torch(w, v, th, torch.from_numpy(x_np).to(dtype))
        (T * torch.from_numpy(g_np).to(dtype)).sum().backward()
        return T.detach().double(), torch.cat([w.grad, v.grad, th.grad.reshape(1)]).double()

    T64, g64 = cpu(torch.float64)
    T32, g32 = cpu(torch.float32)
    cam = utils.CameraTransf()
    with torch.no_grad():
        cam.w.copy_(torch.from_numpy(w_np)); cam.v.copy_(torch.from_numpy(v_np)); cam.theta.copy_(torch.from_numpy(th_np))
    cam = cam.to(dev)
    x = torch.from_numpy(x_np).to(dev).requires_grad_(True)
    T = cam(x)
    assert T.shape == (4, 4) and T.dtype == torch.float32
    (T * torch.from_numpy(g_np).to(dev)).sum().backward()
    assert x.grad is None
    got_T = T.detach().cpu().double()
    got_g = torch.cat([cam.w.grad, cam.v.grad, cam.theta.grad.reshape(1)]).cpu().double()
    assert cam.theta.grad.shape == ()
    err, err32 = float((got_T - T64).abs().max()), float((T32 - T64).abs().max())
    floor = 4 * float(np.spacing(np.float32(T64.abs().max())))
    rel, rel32 = float((got_g - g64).norm() / g64.norm()), float((g32 - g64).norm() / g64.norm())
    print("%s forward: max |T - fp64| kernel %.3e, fp32 torch %.3e (floor %.3e)" % (which, err, err32, floor))
    print("%s backward: rel L2 vs fp64 autograd kernel %.3e, fp32 autograd %.3e" % (which, rel, rel32))
    assert err <= max(2 * err32, floor)
    assert rel <= max(2 * rel32, 1e-6)
    assert torch.equal(T.detach()[3], x.detach()[3])                    # exp_i[3] = (0, 0, 0, 1)


def test_adam_steps_the_zero_dim_theta(dev):
    """optim.Adam over CameraTransf's parameters (theta is 0-dim) against torch.optim.Adam on the CPU, three steps."""
    from nerf_shared_amd import optim, utils
    torch.manual_seed(3)
    cam = utils.CameraTransf()
    twin = [p.detach().clone().requires_grad_(True) for p in cam.parameters()]
    cam = cam.to(dev)
    mine, ref = optim.Adam(cam.parameters(), lr=0.01, betas=(0.9, 0.999)), torch.optim.Adam(twin, lr=0.01, betas=(0.9, 0.999))
    rng = np.random.default_rng(2)
    for _ in range(3):
        for p, q in zip(cam.parameters(), twin):
            g = torch.from_numpy(rng.normal(size=tuple(p.shape)).astype(np.float32)).reshape(p.shape)
            p.grad, q.grad = g.to(dev), g.clone()
        mine.step(); ref.step()
    for p, q in zip(cam.parameters(), twin):
        assert p.shape == q.shape
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().numpy(), rtol=1e-5, atol=1e-9)


# ------------------------------------------------------------------------------------------------ 5. inputs-only backward
def frozen_pair(dev, arch, precision, sharpen, seeds=(1, 11)):
    from nerf_shared_amd import nerf
    ms = []
    for seed in seeds:
        m = nerf.NeRF(**arch)
        m.load_state_dict(synth.torch_state_dict(seed, sharpen, **{**arch, "skips": tuple(arch["skips"])}))
        m = m.to(dev)
        m.precision = precision
        ms.append(m)
    return ms


SMALL = dict(VD, D=4, W=128, skips=[2])


@pytest.mark.parametrize("precision,arch", [("fp32_split", VD), ("bf16", VD), ("fp32", SMALL)], ids=["fp32_split", "bf16", "fp32_D4_W128"])
def test_frozen_models_take_the_inputs_only_backward(dev, precision, arch, monkeypatch):
    """The setting of test_ray_gradients_for_pose_estimation_match_fp32_autograd (80 rays, 32 + 48 samples, both passes):
    dL/d(rays_o, rays_d) with frozen parameters (nerf_amd_field_backward_inputs) against the same with parameters that
    require grad (nerf_amd_field_backward).  Both accumulate ray gradients with float atomics; the yardstick is the
    relative L2 between two runs of the existing path, the gate 4x that (floor 1e-6).  The frozen run leaves every p.grad
    None and never calls nerf_amd_field_backward."""
    from nerf_shared_amd import render_utils
    batch, target = _batch(80, 7)
    r = render_utils.Renderer(**dict(BASE, N_samples=32, N_importance=48))
    mc, mf = frozen_pair(dev, arch, precision, 2.0)
    t = target.to(dev)

    def assemble(o, d):                            # Renderer.render's batch assembly (render_utils.py:205-226)
        vdir = d / torch.norm(d, dim=-1, keepdim=True)
        return torch.cat([o, d, 2.0 * torch.ones_like(d[:, :1]), 6.0 * torch.ones_like(d[:, :1]), vdir], -1)

    def ray_grads(frozen):
        for m in (mc, mf):
            m.requires_grad_(not frozen)
            for p in m.parameters():
                p.grad = None
        ro = batch[:, 0:3].clone().to(dev).requires_grad_(True)
        rd = (batch[:, 3:6] * 1.3).clone().to(dev).requires_grad_(True)
        out = r.render_rays(assemble(ro, rd), mc, mf)
        (((out["rgb_map"] - t) ** 2).mean() + ((out["rgb0"] - t) ** 2).mean()).backward()
        return torch.cat([ro.grad, rd.grad], -1)

    first, second = ray_grads(False), ray_grads(False)
    assert all(p.grad is not None for m in (mc, mf) for p in m.parameters())
    yard = rel_err(second, first)

    def refuse(*a, **k):
        raise AssertionError("nerf_amd_field_backward was called for frozen parameters")
    monkeypatch.setattr(_lib.lib, "nerf_amd_field_backward", refuse)
    got = ray_grads(True)
    assert all(p.grad is None for m in (mc, mf) for p in m.parameters())
    dist = rel_err(got, first)
    print("%s: frozen vs trainable ray gradients rel L2 %.3e; two trainable runs %.3e" % (precision, dist, yard))
    assert torch.isfinite(got).all() and float(got.abs().max()) > 0
    assert dist <= max(4 * yard, 1e-6)


def test_field_backward_still_refuses_null_tables(dev):
    """nerf_amd_field_backward keeps its EINVAL on NULL gradient tables (the inputs-only entry point is a new function)."""
    mc, _ = frozen_pair(dev, VD, "bf16", 1.0)
    h = mc._model_handle(dev, _lib.TRAIN_COPIES[_lib.PREC_BF16])
    rc = _lib.lib.nerf_amd_field_backward(h, None, None, None, None, 11, None, 4, 8, None, 0, None, None, 12, None, None, None,
                                          _lib.PREC_BF16, _lib.stream_of(dev))
    assert rc == -1


# ------------------------------------------------------------------------------------------------ 6. the captured step
TWIST = dict(w=[0.30, -0.25, 0.35], v=[0.30, -0.20, 0.25], theta=0.2)
LOCKSTEP_REPEATS = 3


@pytest.mark.parametrize("start", ["twist_in_module", "demo_init"])
@pytest.mark.parametrize("precision", ["fp32_split", "bf16"])
def test_captured_pose_step_equals_the_eager_loop(dev, precision, start):
    """utils.CapturedPoseStep against the same loop run eagerly on the new ops (cam_transf -> get_rays_at -> render_from_rays
    -> img2mse(rgb) -> backward -> Adam), 12 steps with the demo's learning-rate schedule (lrate 0.01, x 0.8 ** ((k + 1) / 100))
    and a different 64-pixel subset of a 20 x 20 image each step.  Smooth synthetic fields (scale 1.0, the density bias raised
    by 1 so that the volume is a fog with structure instead of empty space: a sharp trained field turns one ulp of a ray into
    1e-3 of gradient, test_pose_optimisation_follows_the_fp32_oracle), perturb 0, the target the render at LEGO_C2W.  The start
    is the target pose moved by the known twist TWIST (rotation 0.1 rad, translation 0.09), in two set-ups:
      demo_init        the demo's own: start_pose = exp(TWIST) @ LEGO_C2W, the module at its normal(0, 1e-6) initialisation
                       (theta -> 0 takes the series branch of theta - sin(theta)).  There the pose is bilinear in (theta, w)
                       and (theta, v) -- every derivative is ~1e-6 of a gradient, below Adam's eps -- and twelve steps move the
                       seven numbers to ~1e-5: the loss cannot be expected to fall, so (e) is left to the other set-up;
      twist_in_module  start_pose = LEGO_C2W and the module's parameters AT the twist: every derivative is informative from
                       the first step and the loss falls.

    What two runs of this loop can be compared on.  The forward is deterministic; the field backward adds ray gradients with
    float atomics, so two runs from ONE state differ in the last bits of the gradient (~1e-7).  Left running freely, that
    difference does not stay small and does not behave like noise with a scale: a last-bit difference in the pose moves, now
    and then, a fine sample across a bin edge (sample_pdf), and the trajectories continue on another BRANCH.  Measured on
    MI355X over 6 fresh processes x 5 runs each: the distance between two free runs takes a few discrete values (fp32_split,
    demo_init: parameters 1e-7 or 2.8e-4, losses 0 or 3.6e-6; bf16: up to 6e-3), whichever pair is eager or captured -- four
    eager runs can share a branch that the fifth run, eager or captured, leaves.  No multiple of a spread sampled from a few
    runs bounds that, so the free-running comparison below is a coarse guard and the sharp comparison is made step by step
    from EQUAL states, where no branch can be taken (the forward sees identical numbers):
    (a) one eager run E is recorded: per step the state before it (seven parameters, both moments, step count), its loss and
        the update it made.  LOCKSTEP_REPEATS more eager passes redo every step from E's recorded state: their largest distance
        from E (loss: relative; update: relative L2 of the seven differences) is the run-to-run spread;
    (b) the captured step, replayed from E's recorded states in the same way (parameters, moments and the host / device step
        count are set before each replay; pixels, target and learning rate as in E): <= 4x that spread, floor rtol 2e-5 (the
        captured training step's gate), for every step's loss and update.  On the update a learning rate that missed one decay
        (0.22 %) or a step count off by one shows a hundred times above the floor;
    free run (12 replays in a row, nothing set in between):
    (c) constructing the step leaves parameters, moments and step count untouched;
    (d) the step count is 12 afterwards, on host and device;
    (e) twist_in_module, fp32_split: the last loss is below the first;
    (f) step.pose equals cam_transf(start_pose) evaluated eagerly after the loop;
    (g) the first loss equals E's (same state, deterministic forward) and the seven parameters end within 5 % of the distance
        Adam can travel (sum of the learning rates: |update| <= lr per step once the moments are warm) of E's -- the guard
        against a free run that goes somewhere else; branches (above) measure up to 1.2 % of it."""
    from nerf_shared_amd import optim, render_utils, utils
    H = W = 20
    K = synth.lego_intrinsics(H, W)
    steps, n, lrate = 12, 64, 0.01
    lr_at = lambda k: lrate * (0.8 ** (k / 100))          # noqa: E731  (the rate step k runs with: set after step k - 1)
    r = render_utils.Renderer(**dict(BASE, N_samples=32, N_importance=32))
    mc, mf = frozen_pair(dev, VD, precision, 1.0, seeds=(0, 10))
    with torch.no_grad():
        for m in (mc, mf):
            m.alpha_linear.bias += 1.0         # (at scale 1.0 every sigma is negative: an empty scene, a white image, a zero loss)
    mc.requires_grad_(False)
    mf.requires_grad_(False)
    target_pose = torch.from_numpy(lego44()).to(dev)
    with torch.no_grad():
        image = r.render_from_pose(H, W, K, 32768, target_pose[:3], mc, mf, retraw=False)[0]
    if start == "demo_init":
        moved = se3_torch(torch.tensor(TWIST["w"], dtype=torch.float64), torch.tensor(TWIST["v"], dtype=torch.float64),
                          torch.tensor(TWIST["theta"], dtype=torch.float64), torch.from_numpy(lego44()).double())
        start_pose = moved.float().to(dev)
        torch.manual_seed(7)
        init = [p.detach().clone() for p in utils.CameraTransf().parameters()]          # normal(0, 1e-6)
        assert max(float(p.abs().max()) for p in init) < 1e-4
    else:
        start_pose = target_pose
        init = [torch.tensor(TWIST["w"]), torch.tensor(TWIST["v"]), torch.tensor(TWIST["theta"])]
    rng = np.random.default_rng(12)
    batches = []
    for _ in range(steps):
        idx = rng.choice(H * W, size=n, replace=False)
        pix = torch.from_numpy(np.stack([idx % W, idx // W], -1)).to(dev)
        batches.append((pix, image[pix[:, 1], pix[:, 0]].contiguous()))

    def fresh():
        cam = utils.CameraTransf()
        with torch.no_grad():
            for p, p0 in zip(cam.parameters(), init):
                p.copy_(p0)
        cam = cam.to(dev)
        return cam, optim.Adam(cam.parameters(), lr=lrate, betas=(0.9, 0.999))

    def seven(cam):
        return torch.cat([cam.w.detach(), cam.v.detach(), cam.theta.detach().reshape(1)]).cpu().double().numpy()

    def set_lr(opt, k):
        for g in opt.param_groups:
            g["lr"] = lr_at(k)

    def eager_step(cam, opt, k):
        pix, tgt = batches[k]
        set_lr(opt, k)
        opt.zero_grad()
        ro, rd = utils.get_rays_at(H, W, K, cam(start_pose), pix)
        rgb = r.render_from_rays(H, W, K, 32768, torch.stack([ro, rd], 0), mc, mf, retraw=True)[0]
        loss = utils.img2mse(rgb, tgt)
        loss.backward()
        opt.step()
        return float(loss.detach())

    def load(cam, opt, state, k):
        """E's state before step k (k >= 1) into a module and its optimizer: parameters, moments, step count."""
        with torch.no_grad():
            for p, (p0, m0, v0) in zip(cam.parameters(), state):
                p.copy_(p0)
                opt.state[p]["exp_avg"].copy_(m0)
                opt.state[p]["exp_avg_sq"].copy_(v0)
        opt._together[0]["step"] = k
        if opt._device_scalars is not None:
            opt._device_scalars[0][0].fill_(k)

    # E: the recorded eager run
    cam, opt = fresh()
    states, losses_e, updates_e = [None], [], []
    for k in range(steps):
        if k > 0:
            states.append([(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in cam.parameters()])
        p0 = seven(cam)
        losses_e.append(eager_step(cam, opt, k))
        updates_e.append(seven(cam) - p0)
    losses_e, final_e = np.array(losses_e), seven(cam)

    def lockstep(cam, opt, one_step):
        """Every step redone from E's state before it: (largest relative loss distance, largest relative L2 distance of the
        update) from E, over the steps."""
        worst_l = worst_u = 0.0
        for k in range(steps):
            if k > 0:
                load(cam, opt, states[k], k)
            p0 = seven(cam)
            loss = one_step(k)
            upd = seven(cam) - p0
            worst_l = max(worst_l, abs(loss - losses_e[k]) / abs(losses_e[k]))
            worst_u = max(worst_u, float(np.linalg.norm(upd - updates_e[k]) / np.linalg.norm(updates_e[k])))
        return worst_l, worst_u

    repeats = []                                                                                                     # (a)
    for _ in range(LOCKSTEP_REPEATS):
        cam, opt = fresh()
        repeats.append(lockstep(cam, opt, lambda k: eager_step(cam, opt, k)))
    spread_l, spread_u = max(d[0] for d in repeats), max(d[1] for d in repeats)

    cam, opt = fresh()
    before = [p.detach().clone() for p in cam.parameters()]
    step = utils.CapturedPoseStep(r, H, W, K, 32768, mc, mf, cam, start_pose, opt, n)
    assert all(torch.equal(p, b) for p, b in zip(cam.parameters(), before))                                          # (c)
    assert opt._together[0]["step"] == 0 and int(opt._device_scalars[0][0]) == 0
    assert all(not st["exp_avg"].any() and not st["exp_avg_sq"].any() for st in opt.state.values())
    assert torch.equal(step.pose, cam(start_pose).detach())

    def replay(k):
        set_lr(opt, k)
        return float(step(*batches[k]))

    got = []                                                         # the free run
    for k in range(steps):
        got.append(replay(k))
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in cam.parameters())
    got, final_c = np.array(got), seven(cam)
    assert opt._together[0]["step"] == steps == int(opt.state_dict()["state"][0]["step"])                            # (d)
    assert int(opt._device_scalars[0][0]) == steps
    with torch.no_grad():
        assert torch.equal(step.pose, cam(start_pose))                                                               # (f)
    travel = sum(lr_at(k) for k in range(steps))
    free_p = float(np.abs(final_c - final_e).max())
    print("eager   ", ["%.4e" % v for v in losses_e])
    print("captured", ["%.4e" % v for v in got])
    print("%s %s free run: first loss captured %.9e eager %.9e; max |parameter difference| %.3e = %.3e of the travel %.3e"
          % (precision, start, got[0], losses_e[0], free_p, free_p / travel, travel))
    print("parameters: start", np.array2string(seven(fresh()[0]), precision=3), "eager", np.array2string(final_e, precision=3),
          "captured", np.array2string(final_c, precision=3))
    assert abs(got[0] - losses_e[0]) <= 2e-5 * abs(losses_e[0])                                                      # (g)
    assert free_p <= 0.05 * travel
    if precision == "fp32_split" and start == "twist_in_module":
        assert got[-1] < got[0] and losses_e[-1] < losses_e[0]                                                       # (e)
    assert not np.array_equal(final_c, seven(fresh()[0])), "degenerate test: the replays did not move the pose"
    assert float(image.std()) > 1e-3 and losses_e[0] > 1e-7, "degenerate test: a featureless target"

    with torch.no_grad():                                            # (b): the same captured step, from E's states
        for p, p0 in zip(cam.parameters(), init):
            p.copy_(p0.to(dev))
        for st in opt.state.values():
            st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
    opt._together[0]["step"] = 0
    opt._device_scalars[0][0].fill_(0)
    dist_l, dist_u = lockstep(cam, opt, replay)
    print("eager lockstep repeats (loss, update):", ["%.2e %.2e" % d for d in repeats])
    print("%s %s lockstep: losses: captured vs eager %.3e, eager spread %.3e; updates: %.3e, %.3e" % (precision, start, dist_l, spread_l, dist_u, spread_u))
    assert dist_l <= max(4 * spread_l, 2e-5)
    assert dist_u <= max(4 * spread_u, 2e-5)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(dev):
    from nerf_shared_amd import optim, render_utils, utils
    H = W = 20
    K = synth.lego_intrinsics(H, W)
    r = render_utils.Renderer(**dict(BASE, N_samples=32, N_importance=32))
    mc, mf = frozen_pair(dev, VD, "bf16", 1.0, seeds=(0, 10))
    cam = utils.CameraTransf().to(dev)
    start = torch.from_numpy(lego44()).to(dev)
    mc.requires_grad_(False)
    with pytest.raises(_lib.NerfAmdError, match="requires_grad_"):             # the fine model still asks for gradients
        utils.CapturedPoseStep(r, H, W, K, 32768, mc, mf, cam, start, optim.Adam(cam.parameters(), lr=0.01), 64)
    mf.requires_grad_(False)
    with pytest.raises(_lib.NerfAmdError, match="optim.Adam"):
        utils.CapturedPoseStep(r, H, W, K, 32768, mc, mf, cam, start, torch.optim.Adam(cam.parameters(), lr=0.01), 64)
    for bad in ([[W, 0]], [[0, H]], [[-1, 3]], torch.tensor([[3, 3], [0, H]])):
        with pytest.raises(_lib.NerfAmdError, match="outside"):
            utils.get_rays_at(H, W, K, start, bad)
    with pytest.raises(_lib.NerfAmdError):
        utils.get_rays_at(H, W, K, start.cpu(), [[0, 0]])                      # the pose must be on the device
