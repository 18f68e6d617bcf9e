"""GPU tests (-m gpu) of multi-start pose estimation: B pose hypotheses in one captured step.

The three batched kernel pairs (se(3), rays at shared pixels, per-hypothesis loss) share their device bodies with the
single-pose kernels, so their oracle is in the repository: slice b of every result is compared with a call of the existing
entry point on slice b, torch.equal.  The captured multi-step (utils.CapturedMultiPoseStep) is compared with B eager loops on
the EXISTING single-pose ops, step by step from equal states, against the run-to-run spread of those loops (the yardstick,
gate and floor of test_captured_pose_step_equals_the_eager_loop, whose docstring says what two runs of this loop can be
compared on and why)."""
import ctypes
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
pytestmark = pytest.mark.gpu

from nerf_shared_amd import _lib, synth  # noqa: E402
from test_gpu_backward import BASE, VD  # noqa: E402
from test_gpu_pose_step import TWIST, frozen_pair, lego44, pixel_cases, pose_grad_reference, se3_params, se3_torch  # noqa: E402

LOCKSTEP_REPEATS = 3
EINVAL = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def k4_of(H, W):
    K = synth.lego_intrinsics(H, W)
    return (ctypes.c_double * 4)(float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))


def poses44(B):
    """[B, 4, 4] float32: the Lego pose, then poses on the camera circle."""
    out = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    out[0] = lego44()
    for b in range(1, B):
        out[b, :3] = synth.pose_spherical(17.0 + 23.0 * b, phi_deg=-30.0 + 2.0 * (b % 5))
    return out


# ------------------------------------------------------------------------------------------------ 1. se(3)
def se3_rows(B):
    """w [B, 3], v [B, 3], theta [B] float32: row 0 at theta 0.3, row 1 with theta == 0 EXACTLY, row 2 at the init scale, row 3 at
    theta 2.5, then those three kinds in turn, each row scaled a little differently so that no two rows are equal."""
    kinds = ["theta_0.3", "zero", "init_scale", "theta_2.5"] + ["theta_0.3", "init_scale", "theta_2.5"] * 67
    w, v, th = np.zeros((B, 3), np.float32), np.zeros((B, 3), np.float32), np.zeros(B, np.float32)
    for b in range(B):
        kind = kinds[b]
        wb, vb, tb = se3_params("theta_2.5" if kind == "zero" else kind)
        s = 1.0 + 0.003 * b
        w[b], v[b], th[b] = np.asarray(wb) * s, np.asarray(vb) / s, 0.0 if kind == "zero" else tb * s
    return w, v, th


@pytest.mark.parametrize("x_mode", ["x_shared", "x_per_hypothesis"])
@pytest.mark.parametrize("B", [1, 2, 5, 64, 65, 200])
def test_se3_batch_equals_the_single_module_bit_for_bit(dev, B, x_mode):
    """CameraTransfBatch(x)[b] and the gradients of row b for a random g_T, torch.equal to a CameraTransf holding row b's
    parameters: 65 and 200 hypotheses need more than one wave, rows cover both branches of theta - sin(theta) and theta == 0."""
    from nerf_shared_amd import utils
    w, v, th = se3_rows(B)
    if B >= 2:
        assert th[1] == 0.0
    x = torch.from_numpy(poses44(B) if x_mode == "x_per_hypothesis" else lego44()).to(dev)
    g_T = torch.from_numpy(np.random.default_rng(B).normal(size=(B, 4, 4)).astype(np.float32)).to(dev)
    cams = utils.CameraTransfBatch(B)
    with torch.no_grad():
        cams.w.copy_(torch.from_numpy(w)); cams.v.copy_(torch.from_numpy(v)); cams.theta.copy_(torch.from_numpy(th))
    cams = cams.to(dev)
    T = cams(x)
    assert T.shape == (B, 4, 4) and T.dtype == torch.float32
    (T * g_T).sum().backward()
    assert cams.w.grad.shape == (B, 3) and cams.v.grad.shape == (B, 3) and cams.theta.grad.shape == (B,)
    assert bool(torch.isfinite(T).all()) and float(cams.w.grad.abs().max()) > 0
    one = utils.CameraTransf().to(dev)
    for b in range(B):
        with torch.no_grad():
            one.w.copy_(cams.w[b]); one.v.copy_(cams.v[b]); one.theta.copy_(cams.theta[b])
        one.w.grad = one.v.grad = one.theta.grad = None
        T1 = one(x[b] if x.dim() == 3 else x)
        (T1 * g_T[b]).sum().backward()
        assert torch.equal(T.detach()[b], T1.detach()), b
        assert torch.equal(cams.w.grad[b], one.w.grad) and torch.equal(cams.v.grad[b], one.v.grad), b
        assert torch.equal(cams.theta.grad[b], one.theta.grad), b
    first = cams.pose_module(0)
    assert torch.equal(first.w, cams.w[0]) and first.w.device == cams.w.device


# ------------------------------------------------------------------------------------------------ 2. rays at shared pixels
RAY_CASES = [c for c in pixel_cases() if c[0] in ("5x7_all_shuffled_plus_duplicates", "800_n1", "800_n65", "800_n1000")]
assert len(RAY_CASES) == 4


@pytest.mark.parametrize("case", RAY_CASES, ids=[c[0] for c in RAY_CASES])
@pytest.mark.parametrize("rows", [3, 4], ids=["c2w_Bx3x4", "c2w_Bx4x4"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_rays_batch_equals_single_bit_for_bit(dev, case, rows, B):
    from nerf_shared_amd import utils
    _, H, W, pix = case
    K = synth.lego_intrinsics(H, W)
    c2w = torch.from_numpy(poses44(B)[:, :rows].copy()).to(dev)
    p = torch.from_numpy(pix).to(dev)
    o, d = utils.get_rays_at(H, W, K, c2w, p)
    assert o.shape == d.shape == (B, pix.shape[0], 3) and o.dtype == d.dtype == torch.float32
    for b in range(B):
        o1, d1 = utils.get_rays_at(H, W, K, c2w[b], p)
        assert torch.equal(o[b], o1) and torch.equal(d[b], d1), b


def rays_bwd_batch(dev, H, W, pix, B, g_o, g_d):
    """nerf_amd_rays_at_pixels_batch_backward, called directly -> (rc, g_c2w [B, 12] prefilled with NaN)."""
    out = torch.full((B, 12), float("nan"), device=dev)
    rc = _lib.lib.nerf_amd_rays_at_pixels_batch_backward(H, W, k4_of(H, W), pix.data_ptr(), pix.shape[0], B, _lib.ptr(g_o), _lib.ptr(g_d),
                                                         out.data_ptr(), _lib.stream_of(dev))
    return rc, out


def rays_bwd_single(dev, H, W, pix, g_o, g_d):
    out = torch.full((12,), float("nan"), device=dev)
    _lib.check(_lib.lib.nerf_amd_rays_at_pixels_backward(H, W, k4_of(H, W), pix.data_ptr(), pix.shape[0], _lib.ptr(g_o), _lib.ptr(g_d),
                                                         out.data_ptr(), None, _lib.stream_of(dev)), "nerf_amd_rays_at_pixels_backward")
    return out


_RNG16K = np.random.default_rng(16)
LIMIT_CASE = ("800_n16384_the_one_block_limit", 800, 800,
              np.stack([_RNG16K.integers(0, 800, size=16384), _RNG16K.integers(0, 800, size=16384)], -1))
BWD_CASES = [(B, c) for B in (1, 3, 8) for c in RAY_CASES] + [(3, LIMIT_CASE)]


@pytest.mark.parametrize("B,case", BWD_CASES, ids=["B%d-%s" % (B, c[0]) for B, c in BWD_CASES])
def test_rays_batch_backward_equals_single_bit_for_bit(dev, B, case):
    """Row b of nerf_amd_rays_at_pixels_batch_backward == nerf_amd_rays_at_pixels_backward on hypothesis b's slices of
    g_rays_o / g_rays_d, with both gradients, with g_o = None and with g_d = None; two calls give equal bits.  (16384 pixels
    are the largest n of one block per hypothesis.)"""
    name, H, W, pix = case
    n = pix.shape[0]
    rng = np.random.default_rng(n + B)
    p = torch.from_numpy(pix).to(device=dev, dtype=torch.int32).contiguous()
    g_o = torch.from_numpy(rng.normal(size=(B, n, 3)).astype(np.float32)).to(dev)
    g_d = torch.from_numpy(rng.normal(size=(B, n, 3)).astype(np.float32)).to(dev)
    for tag, (a, c) in {"both": (g_o, g_d), "g_o=None": (None, g_d), "g_d=None": (g_o, None)}.items():
        rc, got = rays_bwd_batch(dev, H, W, p, B, a, c)
        assert rc == 0, (tag, _lib.lib.nerf_amd_last_error())
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0, tag
        for b in range(B):
            ref = rays_bwd_single(dev, H, W, p, None if a is None else a[b], None if c is None else c[b])
            assert torch.equal(got[b], ref), (tag, b)
        rc, again = rays_bwd_batch(dev, H, W, p, B, a, c)
        assert rc == 0 and torch.equal(got, again), tag


def test_rays_batch_backward_limits_and_the_autograd_path(dev):
    """n = 16385 is beyond one block per hypothesis: EINVAL and nothing launched (the output keeps its NaN fill); n = 0 zeroes
    g_c2w; through autograd a [B, 4, 4] pose gets zero bottom rows and the C entry point's top rows."""
    from nerf_shared_amd import utils
    H = W = 800
    B, n = 3, 16385
    pix = torch.zeros(n, 2, dtype=torch.int32, device=dev)
    g = torch.ones(B, n, 3, device=dev)
    rc, out = rays_bwd_batch(dev, H, W, pix, B, g, g)
    torch.cuda.synchronize()
    assert rc == EINVAL and bool(torch.isnan(out).all())
    assert b"16384" in _lib.lib.nerf_amd_last_error()
    rc, out = rays_bwd_batch(dev, H, W, pix[:0], B, None, None)
    assert rc == 0 and not bool(out.any()) and not bool(torch.isnan(out).any())

    _, H, W, pix_np = RAY_CASES[2]
    n = pix_np.shape[0]
    K = synth.lego_intrinsics(H, W)
    rng = np.random.default_rng(5)
    co = torch.from_numpy(rng.normal(size=(B, n, 3)).astype(np.float32)).to(dev)
    cd = torch.from_numpy(rng.normal(size=(B, n, 3)).astype(np.float32)).to(dev)
    p = torch.from_numpy(pix_np).to(device=dev, dtype=torch.int32).contiguous()
    for rows in (3, 4):
        c2w = torch.from_numpy(poses44(B)[:, :rows].copy()).to(dev).requires_grad_(True)
        o, d = utils.get_rays_at(H, W, K, c2w, p)
        ((o * co).sum() + (d * cd).sum()).backward()
        assert c2w.grad.shape == (B, rows, 4)
        rc, ref = rays_bwd_batch(dev, H, W, p, B, co, cd)
        assert rc == 0 and torch.equal(c2w.grad[:, :3].reshape(B, 12), ref)
        if rows == 4:
            assert not bool(c2w.grad[:, 3].any())


# ------------------------------------------------------------------------------------------------ 3. per-hypothesis loss
@pytest.mark.parametrize("y_mode", ["target_shared", "target_per_hypothesis"])
@pytest.mark.parametrize("n", [1, 64, 257, 1000, 5461])
@pytest.mark.parametrize("B", [1, 4, 9])
def test_loss_batch_equals_single_bit_for_bit(dev, B, n, y_mode):
    """img2mse_each(x, y)[b] == img2mse(x[b], y_b) and its gradient for a random g [B], torch.equal (m = 3 n values per
    hypothesis; 5461 rays are 16383 values, the last size of the one-block path)."""
    from nerf_shared_amd import utils
    rng = np.random.default_rng(1000 * B + n)
    x = torch.from_numpy(rng.uniform(size=(B, n, 3)).astype(np.float32)).to(dev).requires_grad_(True)
    y = torch.from_numpy(rng.uniform(size=(B, n, 3) if y_mode == "target_per_hypothesis" else (n, 3)).astype(np.float32)).to(dev)
    g = torch.from_numpy(rng.normal(size=B).astype(np.float32)).to(dev)
    out = utils.img2mse_each(x, y)
    assert out.shape == (B,) and type(out.grad_fn).__name__.startswith("_Img2MseEachFn")
    out.backward(g)
    assert float(out.detach().min()) > 0 and float(x.grad.abs().max()) > 0
    for b in range(B):
        xb = x.detach()[b].clone().requires_grad_(True)
        yb = y[b] if y.dim() == 3 else y
        one = utils.img2mse(xb, yb)
        one.backward(g[b])
        assert torch.equal(out.detach()[b], one.detach()), b
        assert torch.equal(x.grad[b], xb.grad), b


def test_loss_batch_beyond_one_block(dev):
    """m = 16385: utils.img2mse_each takes the torch expression, the C entry points return EINVAL."""
    from nerf_shared_amd import utils
    B, m = 2, 16385
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.uniform(size=(B, m)).astype(np.float32)).to(dev).requires_grad_(True)
    y = torch.from_numpy(rng.uniform(size=(m,)).astype(np.float32)).to(dev)
    out = utils.img2mse_each(x, y)
    assert "Img2MseEach" not in type(out.grad_fn).__name__
    assert torch.equal(out.detach(), ((x.detach() - y) ** 2).flatten(1).mean(1))
    res, gx = torch.full((B,), float("nan"), device=dev), torch.full((B, m), float("nan"), device=dev)
    xd = x.detach()
    assert _lib.lib.nerf_amd_img2mse_each(xd.data_ptr(), y.data_ptr(), 0, m, B, res.data_ptr(), _lib.stream_of(dev)) == EINVAL
    assert _lib.lib.nerf_amd_img2mse_each_backward(xd.data_ptr(), y.data_ptr(), 0, m, B, res.data_ptr(), gx.data_ptr(),
                                                   _lib.stream_of(dev)) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(res).all()) and bool(torch.isnan(gx).all())
    # the last size inside the limit goes through the library
    assert type(utils.img2mse_each(x[:, :16384].contiguous(), y[:16384].contiguous()).grad_fn).__name__.startswith("_Img2MseEachFn")


# ------------------------------------------------------------------------------------------------ one pose is B = 1 of each op
# The single-pose and the batch entry points launch the same kernels.  What must NOT follow from that: the batch entry points
# pass no `partials`, so at B = 1 they keep their one-block limits, and the single entry points keep theirs.
_RNG16K1 = np.random.default_rng(161)
PIX_16385 = np.stack([_RNG16K1.integers(0, 800, size=16385), _RNG16K1.integers(0, 800, size=16385)], -1)


def test_b1_does_not_open_the_batch_entry_points_past_their_limits(dev):
    """B = 1 with 16385 values per hypothesis: EINVAL from all three batch entry points that have a limit, nothing launched
    (the outputs keep their NaN fill)."""
    L = _lib.lib
    n = m = 16385
    pix = torch.from_numpy(PIX_16385).to(device=dev, dtype=torch.int32).contiguous()
    g = torch.ones(1, n, 3, device=dev)
    rc, out = rays_bwd_batch(dev, 800, 800, pix, 1, g, g)
    assert rc == EINVAL and b"16384" in L.nerf_amd_last_error()
    x, y = torch.rand(1, m, device=dev), torch.rand(m, device=dev)
    res, gx = torch.full((1,), float("nan"), device=dev), torch.full((1, m), float("nan"), device=dev)
    one = torch.ones(1, device=dev)
    for y_stride in (0, m):
        assert L.nerf_amd_img2mse_each(x.data_ptr(), y.data_ptr(), y_stride, m, 1, res.data_ptr(), _lib.stream_of(dev)) == EINVAL
        assert b"16384" in L.nerf_amd_last_error()
        assert L.nerf_amd_img2mse_each_backward(x.data_ptr(), y.data_ptr(), y_stride, m, 1, one.data_ptr(), gx.data_ptr(),
                                                _lib.stream_of(dev)) == EINVAL
        assert b"16384" in L.nerf_amd_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(res).all()) and bool(torch.isnan(gx).all())


def rays_bwd_single_16385(dev, pix, g_o, g_d, partials):
    """nerf_amd_rays_at_pixels_backward over PIX_16385 -> (rc, g_c2w [12] prefilled with NaN)."""
    out = torch.full((12,), float("nan"), device=dev)
    rc = _lib.lib.nerf_amd_rays_at_pixels_backward(800, 800, k4_of(800, 800), pix.data_ptr(), pix.shape[0], _lib.ptr(g_o), _lib.ptr(g_d),
                                                   out.data_ptr(), _lib.ptr(partials), _lib.stream_of(dev))
    return rc, out


def test_single_rays_backward_at_16385_needs_partials_and_is_the_float64_sum(dev):
    """Two blocks: without `partials` EINVAL and nothing launched; with them, and with either gradient null, the float64 sum
    within the bound of test_rays_at_pixels_backward_is_the_float64_sum_and_order_fixed (1e-5 of the sum of |terms| per entry),
    and two calls give equal bits."""
    n = PIX_16385.shape[0]
    rng = np.random.default_rng(n)
    g_o_np, g_d_np = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
    pix = torch.from_numpy(PIX_16385).to(device=dev, dtype=torch.int32).contiguous()
    g_o, g_d = torch.from_numpy(g_o_np).to(dev), torch.from_numpy(g_d_np).to(dev)
    rc, out = rays_bwd_single_16385(dev, pix, g_o, g_d, None)
    torch.cuda.synchronize()
    assert rc == EINVAL and bool(torch.isnan(out).all())
    assert b"needs the partials buffer" in _lib.lib.nerf_amd_last_error()
    partials = torch.empty(256 * 12, device=dev)
    for tag, (a, c) in {"g_o=None": (None, g_d), "g_d=None": (g_o, None)}.items():
        rc, out = rays_bwd_single_16385(dev, pix, a, c, partials)
        assert rc == 0, (tag, _lib.lib.nerf_amd_last_error())
        got = out.cpu().double().numpy().reshape(3, 4)
        ref, mag = pose_grad_reference(800, 800, PIX_16385, None if a is None else g_o_np, None if c is None else g_d_np)
        err = np.abs(got - ref)
        print("n16385 %s: worst |got - ref| / sum|terms| = %.3e" % (tag, float((err / np.maximum(mag, 1e-300)).max())))
        assert np.isfinite(got).all() and (err <= 1e-5 * mag).all(), (tag, got, ref)
        rc, again = rays_bwd_single_16385(dev, pix, a, c, partials)
        assert rc == 0 and torch.equal(out, again), tag


def test_a_1x4x4_pose_and_a_4x4_pose_give_equal_rays_and_gradients(dev):
    """get_rays_at with a [1, 4, 4] and with a [4, 4] pose that requires grad, 5 pixels of a 20 x 20 image: rays and pose
    gradient equal bit for bit, each in its caller's shape, and row 3 of both gradients zero."""
    from nerf_shared_amd import utils
    Hs = Ws = 20
    K = synth.lego_intrinsics(Hs, Ws)
    pix = torch.tensor([[0, 0], [19, 19], [7, 3], [3, 7], [7, 3]], dtype=torch.int32, device=dev)
    rng = np.random.default_rng(44)
    co = torch.from_numpy(rng.normal(size=(5, 3)).astype(np.float32)).to(dev)
    cd = torch.from_numpy(rng.normal(size=(5, 3)).astype(np.float32)).to(dev)
    one = torch.from_numpy(lego44()).to(dev).requires_grad_(True)
    batch = torch.from_numpy(lego44()[None].copy()).to(dev).requires_grad_(True)
    o1, d1 = utils.get_rays_at(Hs, Ws, K, one, pix)
    oB, dB = utils.get_rays_at(Hs, Ws, K, batch, pix)
    assert o1.shape == d1.shape == (5, 3) and oB.shape == dB.shape == (1, 5, 3)
    assert torch.equal(oB[0], o1) and torch.equal(dB[0], d1)
    ((o1 * co).sum() + (d1 * cd).sum()).backward()
    ((oB[0] * co).sum() + (dB[0] * cd).sum()).backward()
    assert one.grad.shape == (4, 4) and batch.grad.shape == (1, 4, 4)
    assert torch.equal(batch.grad[0], one.grad) and float(one.grad[:3].abs().max()) > 0
    assert not bool(one.grad[3].any()) and not bool(batch.grad[0, 3].any())


# ------------------------------------------------------------------------------------------------ the scene of tests 4 to 8
H = W = 20
N_PIX, STEPS, LRATE = 64, 12, 0.01
_SCENES = {}


def scene(dev, precision):
    """The set-up of test_captured_pose_step_equals_the_eager_loop, once per precision: smooth frozen fields with the density
    bias raised by 1, the target image rendered at LEGO_C2W, 12 batches of 64 distinct pixels."""
    from nerf_shared_amd import render_utils
    if precision not in _SCENES:
        K = synth.lego_intrinsics(H, W)
        r = render_utils.Renderer(**dict(BASE, N_samples=32, N_importance=32))
        mc, mf = frozen_pair(dev, VD, precision, 1.0, seeds=(0, 10))
        with torch.no_grad():
            for m in (mc, mf):
                m.alpha_linear.bias += 1.0
        mc.requires_grad_(False)
        mf.requires_grad_(False)
        target_pose = torch.from_numpy(lego44()).to(dev)
        with torch.no_grad():
            image = r.render_from_pose(H, W, K, 32768, target_pose[:3], mc, mf, retraw=False)[0]
        rng = np.random.default_rng(12)
        batches = []
        for _ in range(STEPS):
            idx = rng.choice(H * W, size=N_PIX, replace=False)
            pix = torch.from_numpy(np.stack([idx % W, idx // W], -1)).to(dev)
            batches.append((pix, image[pix[:, 1], pix[:, 0]].contiguous()))
        assert float(image.std()) > 1e-3, "degenerate test: a featureless target"
        _SCENES[precision] = dict(K=K, r=r, mc=mc, mf=mf, target_pose=target_pose, image=image, batches=batches)
    return _SCENES[precision]


# module rows of B = 3 hypotheses: TWIST, -TWIST (the inverse motion), TWIST with theta halved -- informative from the first step
ROWS = [(TWIST["w"], TWIST["v"], TWIST["theta"]), (TWIST["w"], TWIST["v"], -TWIST["theta"]), (TWIST["w"], TWIST["v"], 0.5 * TWIST["theta"])]


def fresh_batch(dev, lrate=LRATE):
    from nerf_shared_amd import optim, utils
    cams = utils.CameraTransfBatch(len(ROWS))
    with torch.no_grad():
        cams.w.copy_(torch.tensor([r[0] for r in ROWS])); cams.v.copy_(torch.tensor([r[1] for r in ROWS]))
        cams.theta.copy_(torch.tensor([r[2] for r in ROWS]))
    cams = cams.to(dev)
    return cams, optim.Adam(cams.parameters(), lr=lrate, betas=(0.9, 0.999))


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("precision", ["fp32_split", "bf16"])
def test_hypotheses_do_not_see_each_other(dev, precision):
    """One eager pass of the multi-step's body, B = 3, n = 64; then again with hypothesis 0 started somewhere else.  The
    losses of hypotheses 1 and 2 are torch.equal (the forward is deterministic and per-ray); their parameter gradients are
    within the run-to-run spread of two identical passes, gate 4x, floor 2e-5 relative L2 (the field backward sums ray
    gradients with float atomics: the yardstick and floor of test_captured_pose_step_equals_the_eager_loop)."""
    from nerf_shared_amd import utils
    s = scene(dev, precision)
    K, r, mc, mf = s["K"], s["r"], s["mc"], s["mf"]
    pix, tgt = s["batches"][0]
    B = len(ROWS)

    def one_pass(start_poses):
        cams, _ = fresh_batch(dev)
        poses = cams(start_poses)
        ro, rd = utils.get_rays_at(H, W, K, poses, pix)
        rgb = r.render_from_rays(H, W, K, 32768, torch.stack([ro.view(-1, 3), rd.view(-1, 3)], 0), mc, mf, retraw=True)[0]
        losses = utils.img2mse_each(rgb.reshape(B, N_PIX, 3), tgt)
        losses.sum().backward()
        grads = torch.cat([cams.w.grad, cams.v.grad, cams.theta.grad[:, None]], 1).cpu().double().numpy()
        return losses.detach().clone(), grads

    same = s["target_pose"].repeat(B, 1, 1)
    other = same.clone()
    other[0, :3] = torch.from_numpy(synth.pose_spherical(40.0)).to(dev)
    l_a, g_a = one_pass(same)
    l_b, g_b = one_pass(same)
    l_c, g_c = one_pass(other)
    assert torch.equal(l_a, l_b)
    assert not torch.equal(l_c[0], l_a[0]), "degenerate test: hypothesis 0 did not change"
    assert torch.equal(l_c[1:], l_a[1:])
    assert float(l_a.min()) > 1e-7 and np.abs(g_a).min(axis=1).max() > 0
    for b in (1, 2):
        spread, dist = rel_l2(g_b[b], g_a[b]), rel_l2(g_c[b], g_a[b])
        print("%s hypothesis %d: gradient rel L2, other hypothesis 0: %.3e; identical passes: %.3e" % (precision, b, dist, spread))
        assert dist <= max(4 * spread, 2e-5)
    assert rel_l2(g_c[0], g_a[0]) > 1e-2, "degenerate test: hypothesis 0's gradient did not change"


# ------------------------------------------------------------------------------------------------ 5. captured multi-step
@pytest.mark.parametrize("precision", ["fp32_split", "bf16"])
def test_captured_multi_step_equals_b_single_loops(dev, precision):
    """utils.CapturedMultiPoseStep (B = 3) against B eager single-hypothesis loops on the EXISTING ops (CameraTransf, 2-D
    get_rays_at, img2mse, optim.Adam), 12 steps, the demo's schedule, a different 64-pixel subset each step.
    (a) reference E: per hypothesis one recorded eager run (state before each step, loss, update); LOCKSTEP_REPEATS eager redo
        passes from E's states give the run-to-run spread per hypothesis;
    (b) lockstep: the captured multi-step replayed from E's states (all B rows of parameters and moments, host and device
        step count set before each replay): every step's loss within max(4 x spread_l, 2e-5) relative and update within
        max(4 x spread_u, 2e-5) relative L2, for every hypothesis;
    free run, 12 replays: construction left parameters, moments and step counts untouched; the step count is 12 on both
    sides; step.poses equals cam_transfs(start_poses) after the loop; first-step losses within 2e-5 relative of E's; every row
    ends within 5 % of the Adam travel (sum of lr) of E's row; fp32_split: every hypothesis's last loss is below its first."""
    from nerf_shared_amd import optim, utils
    s = scene(dev, precision)
    K, r, mc, mf, batches, start_pose = s["K"], s["r"], s["mc"], s["mf"], s["batches"], s["target_pose"]
    B = len(ROWS)
    lr_at = lambda k: LRATE * (0.8 ** (k / 100))          # noqa: E731  (the rate step k runs with)

    def fresh_single(b):
        cam = utils.CameraTransf()
        with torch.no_grad():
            cam.w.copy_(torch.tensor(ROWS[b][0])); cam.v.copy_(torch.tensor(ROWS[b][1])); cam.theta.copy_(torch.tensor(ROWS[b][2]))
        cam = cam.to(dev)
        return cam, optim.Adam(cam.parameters(), lr=LRATE, betas=(0.9, 0.999))

    def seven(cam):
        return torch.cat([cam.w.detach(), cam.v.detach(), cam.theta.detach().reshape(1)]).cpu().double().numpy()

    def sevens(cams):
        return torch.cat([cams.w.detach(), cams.v.detach(), cams.theta.detach()[:, None]], 1).cpu().double().numpy()       # [B, 7]

    def set_lr(opt, k):
        for g in opt.param_groups:
            g["lr"] = lr_at(k)

    def set_count(opt, k):
        opt._together[0]["step"] = k
        if opt._device_scalars is not None:
            opt._device_scalars[0][0].fill_(k)

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

    # (a) E and its spread, per hypothesis
    states, losses_e, updates_e, final_e = [], np.zeros((STEPS, B)), np.zeros((STEPS, B, 7)), np.zeros((B, 7))
    spread_l, spread_u = np.zeros(B), np.zeros(B)
    for b in range(B):
        cam, opt = fresh_single(b)
        st = [None]
        for k in range(STEPS):
            if k > 0:
                st.append([(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in cam.parameters()])
            p0 = seven(cam)
            losses_e[k, b] = eager_step(cam, opt, k)
            updates_e[k, b] = seven(cam) - p0
        states.append(st)
        final_e[b] = seven(cam)
        for _ in range(LOCKSTEP_REPEATS):
            cam, opt = fresh_single(b)
            for k in range(STEPS):
                if k > 0:
                    with torch.no_grad():
                        for p, (p0, m0, v0) in zip(cam.parameters(), st[k]):
                            p.copy_(p0); opt.state[p]["exp_avg"].copy_(m0); opt.state[p]["exp_avg_sq"].copy_(v0)
                    set_count(opt, k)
                p0 = seven(cam)
                loss = eager_step(cam, opt, k)
                spread_l[b] = max(spread_l[b], abs(loss - losses_e[k, b]) / abs(losses_e[k, b]))
                spread_u[b] = max(spread_u[b], rel_l2(seven(cam) - p0, updates_e[k, b]))
    assert losses_e[0].min() > 1e-7, "degenerate test: a featureless target"          # (the first losses, as in the existing test)

    # the free run
    cams, opt = fresh_batch(dev)
    start = sevens(cams)
    before = [p.detach().clone() for p in cams.parameters()]
    step = utils.CapturedMultiPoseStep(r, H, W, K, 32768, mc, mf, cams, start_pose.repeat(B, 1, 1), opt, N_PIX)
    assert all(torch.equal(p, q) for p, q in zip(cams.parameters(), before))
    assert opt._together[0]["step"] == 0 and int(opt._device_scalars[0][0]) == 0
    assert all(not st["exp_avg"].any() and not st["exp_avg_sq"].any() for st in opt.state.values())
    assert step.poses.shape == (B, 4, 4) and torch.equal(step.poses, cams(step.start_poses).detach())

    def replay(k):
        set_lr(opt, k)
        return step(*batches[k]).cpu().double().numpy()

    got = np.zeros((STEPS, B))
    for k in range(STEPS):
        got[k] = replay(k)
        assert step.losses.shape == (B,)
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in cams.parameters())
    final_c = sevens(cams)
    assert opt._together[0]["step"] == STEPS == int(opt.state_dict()["state"][0]["step"])
    assert int(opt._device_scalars[0][0]) == STEPS
    with torch.no_grad():
        assert torch.equal(step.poses, cams(step.start_poses))
    travel = sum(lr_at(k) for k in range(STEPS))
    for b in range(B):
        free_p = float(np.abs(final_c[b] - final_e[b]).max())
        print("%s hypothesis %d free run: first loss captured %.9e eager %.9e, last %.4e / %.4e; max |parameter difference| %.3e = %.3e of "
              "the travel" % (precision, b, got[0, b], losses_e[0, b], got[-1, b], losses_e[-1, b], free_p, free_p / travel))
        assert abs(got[0, b] - losses_e[0, b]) <= 2e-5 * abs(losses_e[0, b])
        assert free_p <= 0.05 * travel
        if precision == "fp32_split":
            assert got[-1, b] < got[0, b]
        assert not np.array_equal(final_c[b], start[b]), "degenerate test: the replays did not move the pose"

    # (b) the same captured step, from E's states
    def load_all(k):
        with torch.no_grad():
            for i, p in enumerate(cams.parameters()):
                for b in range(B):
                    p0, m0, v0 = states[b][k][i] if k > 0 else (torch.tensor(ROWS[b][i]).to(dev), None, None)
                    p[b].copy_(p0)
                    if k > 0:
                        opt.state[p]["exp_avg"][b].copy_(m0); opt.state[p]["exp_avg_sq"][b].copy_(v0)
                    else:
                        opt.state[p]["exp_avg"][b].zero_(); opt.state[p]["exp_avg_sq"][b].zero_()
        set_count(opt, k)

    dist_l, dist_u = np.zeros(B), np.zeros(B)
    for k in range(STEPS):
        load_all(k)
        p0 = sevens(cams)
        losses = replay(k)
        upd = sevens(cams) - p0
        for b in range(B):
            dist_l[b] = max(dist_l[b], abs(losses[b] - losses_e[k, b]) / abs(losses_e[k, b]))
            dist_u[b] = max(dist_u[b], rel_l2(upd[b], updates_e[k, b]))
    for b in range(B):
        print("%s hypothesis %d lockstep: losses: captured vs eager %.3e, eager spread %.3e; updates: %.3e, %.3e"
              % (precision, b, dist_l[b], spread_l[b], dist_u[b], spread_u[b]))
    for b in range(B):
        assert dist_l[b] <= max(4 * spread_l[b], 2e-5), b
        assert dist_u[b] <= max(4 * spread_u[b], 2e-5), b


# ------------------------------------------------------------------------------------------------ 6. with a sampler
def test_captured_multi_step_with_a_sampler(dev):
    from nerf_shared_amd import optim, utils
    s = scene(dev, "fp32_split")
    B = 2
    sampler = utils.PixelSampler(s["image"], N_PIX, strategy="random", seed=5)
    sampler.draw(); sampler.draw()                                   # not a fresh counter: construction must put THIS back
    draws0 = int(sampler.draw_count)
    assert draws0 == 2
    cams = utils.CameraTransfBatch(B).to(dev)
    opt = optim.Adam(cams.parameters(), lr=LRATE, betas=(0.9, 0.999))
    step = utils.CapturedMultiPoseStep(s["r"], H, W, s["K"], 32768, s["mc"], s["mf"], cams, s["target_pose"], opt, N_PIX, sampler=sampler)
    assert int(sampler.draw_count) == draws0
    twin = utils.PixelSampler(s["image"], N_PIX, strategy="random", seed=5)
    twin.reset(draws0)
    for k in range(4):
        losses = step()
        twin.draw()
        assert int(sampler.draw_count) == draws0 + k + 1
        assert step.pixels is sampler.pixels and torch.equal(step.pixels, twin.pixels) and torch.equal(step.target, twin.target)
        assert losses.shape == (B,) and bool(torch.isfinite(losses).all())
    with pytest.raises(_lib.NerfAmdError):
        step(*s["batches"][0])


# ------------------------------------------------------------------------------------------------ 7. the driver
def test_multistart_driver_selects_the_start_at_the_target(dev):
    """estimate_relative_pose_multistart from [the target pose, exp(TWIST) @ target, exp(-TWIST) @ target] with modules at their
    normal(0, 1e-6) initialisation: twelve steps move the parameters by about 1e-5 (test_captured_pose_step_equals_the_eager_loop,
    demo_init), so hypothesis 0 stays at a loss that is only the training-versus-inference forward difference and the other two
    at their twisted losses."""
    from nerf_shared_amd import utils
    s = scene(dev, "fp32_split")
    t64 = torch.from_numpy(lego44()).double()
    w, v = torch.tensor(TWIST["w"], dtype=torch.float64), torch.tensor(TWIST["v"], dtype=torch.float64)
    th = torch.tensor(TWIST["theta"], dtype=torch.float64)
    starts = torch.stack([t64, se3_torch(w, v, th, t64), se3_torch(w, v, -th, t64)]).float()

    def run():
        torch.manual_seed(21)
        return utils.estimate_relative_pose_multistart(s["mc"], s["mf"], s["r"], s["image"], starts, s["K"], 32768, steps=12, batch_size=N_PIX,
                                                       strategy="random", window=4, seed=9)
    est = run()
    pose, losses = est
    assert losses.shape == (12, 3) and losses.is_cuda and pose.shape == (4, 4) and pose.is_cuda
    assert est.poses.shape == (3, 4, 4) and est.scores.shape == (3,) and est.best.shape == () and est.best.dtype == torch.int64
    assert est.best.is_cuda and est.scores.is_cuda and isinstance(est.step, utils.CapturedMultiPoseStep)
    l = losses.cpu().double().numpy()
    assert np.isfinite(l).all()
    l32 = losses.cpu().numpy()
    want = (((l32[-4] + l32[-3]) + l32[-2]) + l32[-1]) / np.float32(4)          # fp32, oldest first: multistart_scores' defined order
    assert want.dtype == np.float32 and np.array_equal(est.scores.cpu().numpy(), want)
    np.testing.assert_allclose(want, l[-4:].mean(0), rtol=4 * 2.0 ** -24, atol=0)      # ... which is the mean, to fp32 rounding
    assert int(est.best) == int(np.argmin(want))
    assert torch.equal(pose, est.poses[int(est.best)])
    assert torch.equal(est.poses, est.step.poses)
    assert l[0, 0] < 0.1 * l[0, 1:].min(), "degenerate test: the start at the target is not clearly the best"
    assert int(est.best) == 0
    again = run()
    assert torch.equal(again.losses[0], losses[0])


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_multipose_refusals(dev):
    from nerf_shared_amd import optim, render_utils, utils
    K = synth.lego_intrinsics(H, W)
    r = render_utils.Renderer(**dict(BASE, N_samples=32, N_importance=32))
    mc, mf = frozen_pair(dev, VD, "bf16", 1.0, seeds=(0, 10))
    cams = utils.CameraTransfBatch(3).to(dev)
    start = torch.from_numpy(lego44()).to(dev)
    adam = lambda ps: optim.Adam(ps, lr=0.01)          # noqa: E731
    mc.requires_grad_(False)
    with pytest.raises(_lib.NerfAmdError, match="requires_grad_"):             # the fine model still asks for gradients
        utils.CapturedMultiPoseStep(r, H, W, K, 32768, mc, mf, cams, start, adam(cams.parameters()), 64)
    mf.requires_grad_(False)
    with pytest.raises(_lib.NerfAmdError, match="optim.Adam"):
        utils.CapturedMultiPoseStep(r, H, W, K, 32768, mc, mf, cams, start, torch.optim.Adam(cams.parameters(), lr=0.01), 64)
    with pytest.raises(_lib.NerfAmdError, match="exactly"):
        utils.CapturedMultiPoseStep(r, H, W, K, 32768, mc, mf, cams, start, adam([cams.w, cams.v]), 64)
    with pytest.raises(_lib.NerfAmdError, match="exactly"):
        utils.CapturedMultiPoseStep(r, H, W, K, 32768, mc, mf, cams, start, adam(utils.CameraTransfBatch(3).to(dev).parameters()), 64)
    with pytest.raises(_lib.NerfAmdError, match="start_poses"):
        utils.CapturedMultiPoseStep(r, H, W, K, 32768, mc, mf, cams, start.repeat(2, 1, 1), adam(cams.parameters()), 64)
    one = utils.CameraTransf().to(dev)
    with pytest.raises(_lib.NerfAmdError, match="CameraTransfBatch"):
        utils.CapturedMultiPoseStep(r, H, W, K, 32768, mc, mf, one, start, adam(one.parameters()), 64)
    sampler = utils.PixelSampler(torch.rand(H, W, 3, device=dev), 32, strategy="random")
    with pytest.raises(_lib.NerfAmdError, match="sampler"):
        utils.CapturedMultiPoseStep(r, H, W, K, 32768, mc, mf, cams, start, adam(cams.parameters()), 64, sampler=sampler)
    with pytest.raises(_lib.NerfAmdError):
        utils.get_rays_at(H, W, K, start.repeat(3, 1, 1).cpu(), [[0, 0]])      # the poses must be on the device
    with pytest.raises(_lib.NerfAmdError):
        utils.get_rays_at(H, W, K, start[None, :2], [[0, 0]])                  # [1, 2, 4]
    with pytest.raises(_lib.NerfAmdError):
        cams(start.repeat(2, 1, 1))
    with pytest.raises(_lib.NerfAmdError):
        utils.estimate_relative_pose_multistart(mc, mf, r, torch.rand(H, W, 3, device=dev), start, K, 32768, steps=1, batch_size=8)

    # the C entry points refuse B = 0 and B = 1025 before any launch (buffers sized for one hypothesis stay untouched)
    L, st = _lib.lib, _lib.stream_of(dev)
    k4 = k4_of(H, W)
    f = lambda *shape: torch.full(shape, float("nan"), device=dev)          # noqa: E731
    wv, th, x, T = f(3), f(1), f(16), f(16)
    pix, rays, g12, m3 = torch.zeros(4, 2, dtype=torch.int32, device=dev), f(4, 3), f(12), f(12)
    for B in (0, 1025, -1):
        assert L.nerf_amd_se3_transform_batch(wv.data_ptr(), wv.data_ptr(), th.data_ptr(), x.data_ptr(), 0, B, T.data_ptr(), st) == EINVAL
        assert L.nerf_amd_se3_transform_batch_backward(wv.data_ptr(), wv.data_ptr(), th.data_ptr(), x.data_ptr(), 0, B, T.data_ptr(),
                                                       wv.data_ptr(), wv.data_ptr(), th.data_ptr(), st) == EINVAL
        assert L.nerf_amd_rays_at_pixels_batch(H, W, k4, x.data_ptr(), 16, 4, B, pix.data_ptr(), 4, rays.data_ptr(), rays.data_ptr(), st) == EINVAL
        assert L.nerf_amd_rays_at_pixels_batch_backward(H, W, k4, pix.data_ptr(), 4, B, rays.data_ptr(), rays.data_ptr(), g12.data_ptr(), st) == EINVAL
        assert L.nerf_amd_img2mse_each(m3.data_ptr(), m3.data_ptr(), 0, 12, B, th.data_ptr(), st) == EINVAL
        assert L.nerf_amd_img2mse_each_backward(m3.data_ptr(), m3.data_ptr(), 0, 12, B, th.data_ptr(), m3.data_ptr(), st) == EINVAL
        assert b"1024" in L.nerf_amd_last_error()
    # null pointers, a stride that is neither shared nor dense
    assert L.nerf_amd_se3_transform_batch(None, wv.data_ptr(), th.data_ptr(), x.data_ptr(), 0, 1, T.data_ptr(), st) == EINVAL
    assert L.nerf_amd_se3_transform_batch(wv.data_ptr(), wv.data_ptr(), th.data_ptr(), x.data_ptr(), 4, 1, T.data_ptr(), st) == EINVAL
    assert L.nerf_amd_rays_at_pixels_batch(H, W, k4, x.data_ptr(), -16, 4, 1, pix.data_ptr(), 4, rays.data_ptr(), rays.data_ptr(), st) == EINVAL
    assert L.nerf_amd_rays_at_pixels_batch_backward(H, W, k4, pix.data_ptr(), 4, 1, rays.data_ptr(), rays.data_ptr(), None, st) == EINVAL
    assert L.nerf_amd_img2mse_each(m3.data_ptr(), m3.data_ptr(), 5, 12, 1, th.data_ptr(), st) == EINVAL
    assert L.nerf_amd_img2mse_each_backward(m3.data_ptr(), m3.data_ptr(), 0, 12, 1, None, m3.data_ptr(), st) == EINVAL
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (wv, th, x, T, rays, g12, m3))
