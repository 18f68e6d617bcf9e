"""GPU tests (-m gpu) of joint training of the field and the camera poses: rays whose pose differs per ray
(utils.get_rays_indexed over nerf_amd_rays_at_pixels_indexed), se(3) twists (utils.SE3Twist / utils.LearnedPoses over
nerf_amd_se3_exp_batch), the image-bank draw (utils.ImageBankSampler) and the captured step (utils.CapturedJointStep).

Every bound is exact (torch.equal), derived from the number formats, a gate an existing test file already holds the same
code to, or a multiple of a yardstick measured in the same test -- never a number taken from the code under test."""
import ctypes
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
pytestmark = pytest.mark.gpu

from nerf_shared_amd import _lib, synth  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402
from test_gpu_backward import BASE, VD, bf16_field, rel_err  # noqa: E402
from test_gpu_pose_step import lego44, pose_grad_reference  # noqa: E402
from test_gpu_split_backward import assert_table, check_params, cosine, models, oracle_two_pass  # noqa: E402

SIZES = [1, 63, 64, 65, 1000, 1025, 16385]        # the wave boundary, the block boundary, the batch form's one-block limit
POSE_COUNTS = [1, 3, 64, 65]
IMAGES = [(5, 7), (400, 400)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def k4_of(H, W):
    K = synth.lego_intrinsics(H, W)
    return (ctypes.c_double * 4)(float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))


def pose_table(M, seed=5):
    """M distinct camera poses [M, 4, 4] float32 (numpy): LEGO_C2W and M - 1 rigid perturbations of it."""
    from nerf_shared_amd import utils
    return utils.perturbed_start_poses(lego44(), M, 8.0, 0.15, seed=seed)


def mixed_batch(H, W, M, n, seed):
    """n random pixels (x, y) [n, 2] and a random pose per ray [n], int64 numpy; every pose has a ray where n allows."""
    rng = np.random.default_rng(seed)
    pix = np.stack([rng.integers(0, W, size=n), rng.integers(0, H, size=n)], -1)
    p = rng.integers(0, M, size=n)
    p[:min(n, M)] = rng.permutation(M)[:min(n, M)]
    return pix, p


# ------------------------------------------------------------------------------------------------ 1. indexed rays, forward
@pytest.mark.parametrize("layout", ["M34", "M44", "row_strided", "pose_strided"])
@pytest.mark.parametrize("M", POSE_COUNTS)
@pytest.mark.parametrize("HW", IMAGES, ids=["5x7", "400x400"])
def test_indexed_rays_equal_the_single_pose_rays_bit_for_bit(dev, HW, M, layout):
    """Row i of get_rays_indexed equals get_rays_at with pose p_i at pixel i (torch.equal), for every n of SIZES, with the
    table as [M, 3, 4], [M, 4, 4], a view with a row stride of 8 floats and a view that takes every other pose; the
    stacked-row mode (pose_index None, y = p H + row) gives the same bits."""
    from nerf_shared_amd import utils
    H, W = HW
    K = synth.lego_intrinsics(H, W)
    table = torch.from_numpy(pose_table(M)).to(dev)
    if layout == "M34":
        c2w = table[:, :3].contiguous()
    elif layout == "M44":
        c2w = table
    elif layout == "row_strided":
        wide = torch.full((M, 4, 8), 777.0, device=dev)
        wide[:, :, :4] = table
        c2w = wide[:, :, :4]
    else:
        twice = torch.full((2 * M, 4, 4), 777.0, device=dev)
        twice[::2] = table
        c2w = twice[::2]
    assert layout in ("M34", "M44") or not c2w.is_contiguous() or (layout == "pose_strided" and M == 1)   # (one pose has no pose stride)
    for n in SIZES:
        pix_np, p_np = mixed_batch(H, W, M, n, seed=n + M)
        pix, p = torch.from_numpy(pix_np).to(dev), torch.from_numpy(p_np).to(dev)
        o, d = utils.get_rays_indexed(H, W, K, c2w, pix, p)
        assert o.shape == d.shape == (n, 3) and o.dtype == d.dtype == torch.float32
        for m in range(M):
            sel = p == m
            if bool(sel.any()):
                o_ref, d_ref = utils.get_rays_at(H, W, K, table[m], pix[sel])
                assert torch.equal(o[sel], o_ref) and torch.equal(d[sel], d_ref), (n, m)
        stacked = torch.stack([pix[:, 0], p * H + pix[:, 1]], -1)
        o2, d2 = utils.get_rays_indexed(H, W, K, c2w, stacked)
        assert torch.equal(o2, o) and torch.equal(d2, d), n
    o3, d3 = utils.get_rays_indexed(H, W, K, c2w, pix_np.tolist(), p_np.tolist())          # host inputs: checked, then the same
    assert torch.equal(o3, o) and torch.equal(d3, d)


# ------------------------------------------------------------------------------------------------ 2. indexed rays, backward
def indexed_bwd(dev, H, W, pix, pose_index, M, g_o, g_d):
    """nerf_amd_rays_at_pixels_indexed_backward, called directly -> [M, 12] (prefilled with NaN: every entry is written)."""
    out = torch.full((M, 12), float("nan"), device=dev)
    _lib.check(_lib.lib.nerf_amd_rays_at_pixels_indexed_backward(H, W, k4_of(H, W), pix.data_ptr(), _lib.ptr(pose_index), pix.shape[0], M,
                                                                 _lib.ptr(g_o), _lib.ptr(g_d), out.data_ptr(), _lib.stream_of(dev)),
               "nerf_amd_rays_at_pixels_indexed_backward")
    return out


def plus_zero(t):
    return bool((t == 0).all()) and not bool(torch.signbit(t).any())


@pytest.mark.parametrize("M,m0", [(1, 0), (3, 1), (65, 64)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 1025, 16384])
def test_indexed_backward_with_every_ray_on_one_pose_is_the_batch_form_at_b1(dev, n, M, m0):
    """All rays on pose m0 (n <= 16384, the batch form's limit): row m0 equals nerf_amd_rays_at_pixels_batch_backward at B = 1 on
    the same buffers bit for bit, every other row is +0.0; with both gradients, g_o = NULL and g_d = NULL; in index mode and in
    stacked-row mode."""
    H, W = 400, 400
    rng = np.random.default_rng(n)
    pix_np, _ = mixed_batch(H, W, 1, n, seed=n)
    pix = torch.from_numpy(pix_np).to(device=dev, dtype=torch.int32).contiguous()
    idx = torch.full((n,), m0, device=dev, dtype=torch.int32)
    stacked = pix.clone()
    stacked[:, 1] += m0 * H
    g_o, g_d = (torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32)).to(dev) for _ in range(2))
    for tag, (a, b) in {"both": (g_o, g_d), "g_o=NULL": (None, g_d), "g_d=NULL": (g_o, None)}.items():
        ref = torch.full((12,), float("nan"), device=dev)
        _lib.check(_lib.lib.nerf_amd_rays_at_pixels_batch_backward(H, W, k4_of(H, W), pix.data_ptr(), n, 1, _lib.ptr(a), _lib.ptr(b),
                                                                   ref.data_ptr(), _lib.stream_of(dev)), "nerf_amd_rays_at_pixels_batch_backward")
        for mode, got in (("index", indexed_bwd(dev, H, W, pix, idx, M, a, b)), ("stacked", indexed_bwd(dev, H, W, stacked, None, M, a, b))):
            assert torch.equal(got[m0], ref), (tag, mode)
            others = torch.cat([got[:m0], got[m0 + 1:]])
            assert plus_zero(others), (tag, mode)


@pytest.mark.parametrize("M", POSE_COUNTS)
@pytest.mark.parametrize("HW", IMAGES, ids=["5x7", "400x400"])
def test_indexed_backward_is_the_float64_sum_per_pose_and_order_fixed(dev, HW, M):
    """Mixed indices at the shapes of the forward test: every row within 1e-5 * sum |terms| of the float64 sum over its own rays
    -- the bound and reasoning of test_rays_at_pixels_backward_is_the_float64_sum_and_order_fixed: a tree sum of fp32 terms
    errs by about log2(n) 2^-24 of that, the margin covers the per-thread serial part (16 terms at n = 16385) and the fp32
    pixel directions.  A pose without rays is +0.0, two calls on equal inputs are torch.equal, and the autograd path gives
    the same rows (row 3 of a [M, 4, 4] table zero)."""
    from nerf_shared_amd import utils
    H, W = HW
    for n in SIZES:
        pix_np, p_np = mixed_batch(H, W, M, n, seed=3 * n + M)
        rng = np.random.default_rng(n)
        g_o_np, g_d_np = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
        pix = torch.from_numpy(pix_np).to(device=dev, dtype=torch.int32).contiguous()
        idx = torch.from_numpy(p_np).to(device=dev, dtype=torch.int32)
        g_o, g_d = torch.from_numpy(g_o_np).to(dev), torch.from_numpy(g_d_np).to(dev)
        got_t = indexed_bwd(dev, H, W, pix, idx, M, g_o, g_d)
        assert torch.equal(got_t, indexed_bwd(dev, H, W, pix, idx, M, g_o, g_d)), n
        got = got_t.cpu().double().numpy().reshape(M, 3, 4)
        worst = 0.0
        for m in range(M):
            sel = p_np == m
            if not sel.any():
                assert plus_zero(got_t[m]), (n, m)
                continue
            ref, mag = pose_grad_reference(H, W, pix_np[sel], g_o_np[sel], g_d_np[sel])
            err = np.abs(got[m] - ref)
            worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
            assert np.isfinite(got[m]).all() and (err <= 1e-5 * mag).all(), (n, m, got[m], ref)
        print("%dx%d M=%d n=%d: worst |got - ref| / sum|terms| = %.3e" % (H, W, M, n, worst))
    table = torch.from_numpy(pose_table(M)).to(dev).requires_grad_(True)
    o, d = utils.get_rays_indexed(H, W, synth.lego_intrinsics(H, W), table, pix, idx)
    ((o * g_o).sum() + (d * g_d).sum()).backward()
    assert table.grad.shape == (M, 4, 4) and torch.equal(table.grad[:, :3].reshape(M, 12), got_t) and not table.grad[:, 3].any()


# ------------------------------------------------------------------------------------------------ 3. the index guard
@pytest.mark.parametrize("mode", ["index", "stacked"])
def test_a_pose_index_outside_the_table_never_forms_an_address(dev, mode):
    """The table is a view into the MIDDLE of a larger tensor whose other rows hold a sentinel, so an unguarded read of pose -1
    or M lands in owned memory and shows.  Rays with index -1 or M (stacked: y < 0 or y >= M H) are NaN; every other ray and
    every gradient row equals, bit for bit, the run in which those rays belong to one MORE pose (a table of M + 1 poses: the
    same thread owns the same ray, so rows 0 .. M-1 see the same sums in the same order); the sentinel never shows."""
    H, W, M, n, SENTINEL = 5, 7, 3, 200, 1.0e6
    big = torch.full((M + 5, 4, 4), SENTINEL, device=dev)
    big[2:2 + M + 1] = torch.from_numpy(pose_table(M + 1)).to(dev)
    inside, one_more = big[2:2 + M], big[2:2 + M + 1]
    big[2 + M] = SENTINEL                                                       # the row behind the table, while M poses are in use
    pix_np, p_np = mixed_batch(H, W, M, n, seed=8)
    bad = np.array([0, 5, 63, 64, 130, 199])
    p_bad = p_np.copy()
    p_bad[bad] = [-1, M, M, -1, M + 1, -(2 ** 31)]
    rng = np.random.default_rng(2)
    g_o, g_d = (torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32)).to(dev) for _ in range(2))
    pix = torch.from_numpy(pix_np).to(device=dev, dtype=torch.int32)
    K = synth.lego_intrinsics(H, W)

    def run(table, p):
        from nerf_shared_amd import utils
        m = table.shape[0]
        p_t = torch.from_numpy(p).to(device=dev, dtype=torch.int32)
        if mode == "index":
            px, idx = pix, p_t
        else:
            # the stacked row that names the same pose; poses outside [-1, M] have no row of their own: y far outside
            y = torch.where((p_t >= -1) & (p_t <= M + 1), p_t * H + pix[:, 1], torch.where(p_t < 0, p_t, p_t.new_tensor(2 ** 31 - 1)))
            px, idx = torch.stack([pix[:, 0], y], -1).contiguous(), None
        o, d = utils.get_rays_indexed(H, W, K, table, px, idx)
        return o, d, indexed_bwd(dev, H, W, px.contiguous(), idx, m, g_o, g_d)

    o, d, g = run(inside, p_bad)
    good = np.setdiff1d(np.arange(n), bad)
    assert bool(torch.isnan(o[bad]).all()) and bool(torch.isnan(d[bad]).all())
    assert bool(torch.isfinite(o[good]).all()) and bool(torch.isfinite(d[good]).all()) and bool(torch.isfinite(g).all())
    assert float(o[good].abs().max()) < 100 and float(d[good].abs().max()) < 100 and float(g.abs().max()) < 1e4      # no sentinel
    big[2 + M] = torch.from_numpy(pose_table(M + 1)[M]).to(dev)
    p_valid = p_np.copy()
    p_valid[bad] = M                                                            # the run without them: they belong to pose M
    o2, d2, g2 = run(one_more, p_valid)
    assert torch.equal(o[good], o2[good]) and torch.equal(d[good], d2[good])
    assert torch.equal(g, g2[:M])
    assert float(g2[M].abs().max()) > 0                                         # (their gradients exist -- and entered no row above)


# ------------------------------------------------------------------------------------------------ 4. the twist
OMEGA_NORMS = [1e-7, 1e-3, 0.0999, 0.1001, 1.0, 3.0]          # the series threshold is |omega| = 0.1 (include/nerf_amd.h)


def twist_rows(M, seed):
    """xi [M, 6] float32: row 0 exactly zero, row 1 a pure translation (omega = 0), then |omega| cycling through OMEGA_NORMS in
    random directions with upsilon ~ 0.5 N(0, 1)."""
    rng = np.random.default_rng(seed)
    xi = np.zeros((M, 6), np.float32)
    for m in range(1, M):
        xi[m, 3:] = 0.5 * rng.normal(size=3)
        if m >= 2:
            w = rng.normal(size=3)
            xi[m, :3] = w / np.linalg.norm(w) * OMEGA_NORMS[(m - 2) % len(OMEGA_NORMS)]
    return xi


def exp_reference(xi, X):
    """float64 matrix exponential of the 4 x 4 twist times X: (T [M, 4, 4], J [M, 4, 4, 6] = dT / dxi), torch float64 on the CPU."""
    xi64 = torch.from_numpy(xi).double().requires_grad_(True)
    w, u, z = xi64[:, :3], xi64[:, 3:], torch.zeros(xi.shape[0], dtype=torch.float64)
    A = torch.stack([torch.stack([z, -w[:, 2], w[:, 1], u[:, 0]], -1), torch.stack([w[:, 2], z, -w[:, 0], u[:, 1]], -1),
                     torch.stack([-w[:, 1], w[:, 0], z, u[:, 2]], -1), torch.stack([z, z, z, z], -1)], 1)
    T = torch.linalg.matrix_exp(A) @ torch.from_numpy(X).double()
    J = torch.zeros(xi.shape[0], 4, 4, 6, dtype=torch.float64)
    for i in range(3):
        for j in range(4):
            J[:, i, j] = torch.autograd.grad(T[:, i, j].sum(), xi64, retain_graph=True)[0]
    return T.detach(), J


@pytest.mark.parametrize("shared_x", [False, True], ids=["x_per_pose", "x_shared"])
@pytest.mark.parametrize("M", [1, 5, 64, 65, 200])
def test_twist_matches_the_float64_matrix_exponential(dev, M, shared_x):
    """Forward: per entry |got - ref| <= 2^-23 |ref| + 1e-12 max(1, max |X|) -- one fp32 rounding plus the fp64 evaluation
    error -- against float64 torch.linalg.matrix_exp of the 4 x 4 twist times X, for xi = 0 (bit-equal to X, a -0.0 entry
    included), a pure translation, and |omega| = 1e-7, 1e-3, just below and just above the series threshold 0.1, 1 and 3.
    Backward with a random g_T: against float64 autograd through the same expression, per entry within 2^-23 sum |terms| +
    the same absolute term; at xi = 0 all six derivatives are non-zero."""
    from nerf_shared_amd import utils
    xi_np = twist_rows(M, seed=M)
    X_np = pose_table(M, seed=9)
    X_np[0, 1, 2] = -0.0                                                    # bit for bit means the sign of a zero too
    if shared_x:
        X_np = X_np[0]
    g_np = np.random.default_rng(M + 1).normal(size=(M, 4, 4)).astype(np.float32)
    tw = utils.SE3Twist(M)
    with torch.no_grad():
        tw.xi.copy_(torch.from_numpy(xi_np))
    tw = tw.to(dev)
    X = torch.from_numpy(X_np).to(dev).requires_grad_(True)
    T = tw(X)
    assert T.shape == (M, 4, 4) and T.dtype == torch.float32
    (T * torch.from_numpy(g_np).to(dev)).sum().backward()
    assert X.grad is None and tw.xi.grad.shape == (M, 6)
    x0 = torch.from_numpy(X_np if shared_x else X_np[0]).to(dev)
    assert torch.equal(T[0].view(torch.int32), x0.view(torch.int32)), "xi = 0 must return X bit for bit"
    T_ref, J = exp_reference(xi_np, X_np)
    floor = 1e-12 * max(1.0, float(np.abs(X_np).max()))
    err = (T.detach().cpu().double() - T_ref).abs()
    bound = 2.0 ** -23 * T_ref.abs() + floor
    print("M=%d forward: worst err / bound %.3f" % (M, float((err / bound).max())))
    assert bool((err <= bound).all()), (err / bound).max()
    g64 = torch.from_numpy(g_np).double()
    ref = (g64[..., None] * J).sum((1, 2))
    mag = (g64[..., None] * J).abs().sum((1, 2))
    gerr = (tw.xi.grad.cpu().double() - ref).abs()
    gbound = 2.0 ** -23 * mag + floor
    print("M=%d backward: worst err / bound %.3f" % (M, float((gerr / gbound).max())))
    assert bool((gerr <= gbound).all()), (gerr / gbound).max()
    assert bool((tw.xi.grad[0] != 0).all()), "the derivative at xi = 0 is the six generators applied to X"


def test_learned_poses_keep_frozen_views_exactly(dev):
    """LearnedPoses(frozen=...): frozen rows return the given pose bit for bit -- whatever their xi holds -- and their xi.grad is
    exactly zero; the other rows are SE3Twist's, values and gradients."""
    from nerf_shared_amd import utils
    M, frozen = 6, (1, 4)
    poses = pose_table(M, seed=3)
    xi = twist_rows(M + 2, seed=4)[2:]                                       # every row non-zero, the frozen ones too
    g = torch.from_numpy(np.random.default_rng(6).normal(size=(M, 4, 4)).astype(np.float32)).to(dev)
    lp = utils.LearnedPoses(poses, frozen=frozen)
    fresh = lp.to(dev)()
    assert torch.equal(fresh, torch.from_numpy(poses).to(dev))               # a fresh module: the given poses
    with torch.no_grad():
        lp.twist.xi.copy_(torch.from_numpy(xi))
    out = lp()
    (out * g).sum().backward()
    tw = utils.SE3Twist(M).to(dev)
    with torch.no_grad():
        tw.xi.copy_(torch.from_numpy(xi))
    ref = tw(torch.from_numpy(poses).to(dev))
    (ref * g).sum().backward()
    free = [m for m in range(M) if m not in frozen]
    assert torch.equal(out[list(frozen)], torch.from_numpy(poses[list(frozen)]).to(dev))
    assert bool((lp.twist.xi.grad[list(frozen)] == 0).all())
    assert torch.equal(out[free], ref[free].detach()) and torch.equal(lp.twist.xi.grad[free], tw.xi.grad[free])
    assert bool((lp.twist.xi.grad[free] != 0).any(1).all())


# ------------------------------------------------------------------------------------------------ 5. the joint gradient, eager
H20 = W20 = 20
N_IMAGES, N_RAYS = 4, 64
JOINT_CFG = dict(BASE, N_samples=32, N_importance=32)


def fog_models(dev, precision):
    """The smooth fog fields of test_captured_pose_step_equals_the_eager_loop (scale 1.0, the density bias raised by 1), trainable,
    with their oracle twins: ((coarse, fine), (oracle coarse, oracle fine))."""
    pairs = [models(dev, seed, 1.0, VD, precision) for seed in (0, 10)]
    with torch.no_grad():
        for m, cpu in pairs:
            m.alpha_linear.bias += 1.0
            cpu["alpha_linear.bias"] += 1.0
            m.weights_changed()
    return [p[0] for p in pairs], [p[1] for p in pairs]


_SCENE = {}


def joint_scene(dev):
    """Once per session: M true poses, their 20 x 20 images rendered from the fp32_split fog fields, K, and a 64-ray batch spread
    over the images (pixels, pose index, target)."""
    from nerf_shared_amd import render_utils
    if not _SCENE:
        K = synth.lego_intrinsics(H20, W20)
        r = render_utils.Renderer(**JOINT_CFG)
        (mc, mf), _ = fog_models(dev, "fp32_split")
        poses = pose_table(N_IMAGES, seed=21)
        with torch.no_grad():
            images = torch.stack([r.render_from_pose(H20, W20, K, 32768, torch.from_numpy(p[:3]).to(dev), mc, mf, retraw=False)[0]
                                  for p in poses]).contiguous()
        assert images.shape == (N_IMAGES, H20, W20, 3) and float(images.std()) > 1e-3
        pix_np, p_np = mixed_batch(H20, W20, N_IMAGES, N_RAYS, seed=13)
        pix, p = torch.from_numpy(pix_np).to(dev), torch.from_numpy(p_np).to(dev)
        _SCENE.update(K=K, poses=poses, images=images, pix=pix, p=p, target=images[p, pix[:, 1], pix[:, 0]].contiguous())
    return _SCENE


def assemble(o, d):                            # Renderer.render's batch assembly (render_utils.py:205-226)
    vdir = d / torch.norm(d, dim=-1, keepdim=True)
    return torch.cat([o, d, 2.0 * torch.ones_like(d[:, :1]), 6.0 * torch.ones_like(d[:, :1]), vdir], -1)


@pytest.mark.parametrize("precision", ["fp32_split", "bf16"])
def test_joint_gradients_eager(dev, precision, monkeypatch):
    """One eager joint step's gradients: 20 x 20 images, M = 4, 64 rays spread over the images, 32 + 32 samples, fog fields, poses
    moved by twists of a few degrees.
    fp32_split: field parameter gradients against fp32 autograd on the oracle (on the run's own rays and fine depths) within
    the gates of test_gpu_split_backward.py, rel-L2 <= 1e-3 and cosine >= 0.9999; xi.grad of image m within the same gates of
    the gradient of the same loss restricted to image m's rays, computed through the EXISTING single-pose path (get_rays_at on
    that image's pixels, the loss scaled by n_m / n) and the float64 derivative of the exponential -- the new routing against
    code already held to the oracle.
    bf16: finite, and parameter gradients within the gates of test_gpu_backward.py's training step: rel-L2 <= 8e-2 against
    autograd on the oracle with the kernel's bf16 roundings, cosine >= 0.97 against fp32 autograd."""
    from nerf_shared_amd import render_utils, utils
    s = joint_scene(dev)
    K, pix, p, target = s["K"], s["pix"], s["p"], s["target"]
    r = render_utils.Renderer(**JOINT_CFG)
    (mc, mf), (cc, cf) = fog_models(dev, precision)
    xi0 = (0.04 * np.random.default_rng(31).normal(size=(N_IMAGES, 6))).astype(np.float32)
    lp = utils.LearnedPoses(s["poses"])
    with torch.no_grad():
        lp.twist.xi.copy_(torch.from_numpy(xi0))
    lp = lp.to(dev)
    poses = lp()
    ro, rd = utils.get_rays_indexed(H20, W20, K, poses, pix, p)
    out = r.render_rays(assemble(ro, rd), mc, mf, retweights=True)
    loss = ((out["rgb_map"] - target) ** 2).mean() + ((out["rgb0"] - target) ** 2).mean()
    loss.backward()
    xi_grad = lp.twist.xi.grad.detach().cpu().double()
    assert bool(torch.isfinite(xi_grad).all()) and bool((xi_grad != 0).all())
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for m in (mc, mf) for q in m.parameters())

    batch, z_f, t = assemble(ro.detach().cpu(), rd.detach().cpu()), out["z_vals"].detach().cpu(), target.cpu()

    def oracle_grads(field):
        if field is not None:
            monkeypatch.setattr(O, "nerf_forward", lambda sd, arch, pts, vd, netchunk=0: field(sd, pts, vd))
        c = {k: v.detach().clone().requires_grad_(True) for k, v in cc.items()}
        f = {k: v.detach().clone().requires_grad_(True) for k, v in cf.items()}
        rgb, rgb0 = oracle_two_pass(JOINT_CFG, batch, (c, O.Arch(**VD)), (f, O.Arch(**VD)), z_f)
        l = ((rgb - t) ** 2).mean() + ((rgb0 - t) ** 2).mean()
        l.backward()
        monkeypatch.undo()
        return float(l), c, f

    l32, c32, f32 = oracle_grads(None)
    if precision == "bf16":
        lb, cb, fb = oracle_grads(bf16_field)
        assert abs(float(loss) - lb) < 2e-3 * max(1.0, abs(lb))
        for tag, m, gb, g32 in (("coarse", mc, cb, c32), ("fine", mf, fb, f32)):
            for name, q in m.named_parameters():
                g = q.grad.detach().cpu()
                eb, cos = rel_err(g, gb[name].grad), cosine(g, g32[name].grad)
                print("%-34s err vs bf16-model %.4f   cos fp32 %.5f" % (tag + "." + name, eb, cos))
                assert eb < 8e-2 and cos > 0.97, (tag, name, eb, cos)
        return
    assert abs(float(loss) - l32) < 2e-6 * max(1.0, abs(l32))
    table = []
    check_params("coarse.", mc, c32, table)
    check_params("fine.", mf, f32, table)
    assert_table(table)

    _, J = exp_reference(xi0, s["poses"])                                       # [M, 4, 4, 6], float64
    rows = []
    for m in range(N_IMAGES):
        sel = p == m
        n_m = int(sel.sum())
        assert n_m > 0
        pose_m = poses.detach()[m].clone().requires_grad_(True)
        ro_m, rd_m = utils.get_rays_at(H20, W20, K, pose_m, pix[sel])
        out_m = r.render_rays(assemble(ro_m, rd_m), mc, mf)
        loss_m = (((out_m["rgb_map"] - target[sel]) ** 2).mean() + ((out_m["rgb0"] - target[sel]) ** 2).mean()) * (n_m / N_RAYS)
        loss_m.backward()
        ref = (pose_m.grad.cpu().double()[..., None] * J[m]).sum((0, 1))
        rows.append(("xi.grad[%d] (%d rays)" % (m, n_m), rel_err(xi_grad[m], ref), cosine(xi_grad[m], ref)))
    assert_table(rows)


# ------------------------------------------------------------------------------------------------ 6. captured against eager
LOCKSTEP_REPEATS = 3


@pytest.mark.parametrize("precision", ["fp32_split", "bf16"])
def test_captured_joint_step_equals_the_eager_loop(dev, precision):
    """utils.CapturedJointStep against the same loop run eagerly (learned_poses -> get_rays_indexed -> render_from_rays ->
    img2mse(rgb) + img2mse(rgb0) -> backward -> one Adam over two groups), 8 steps, a different 64-ray batch over the four images
    each step, both learning rates decayed every step, view 0 frozen.  The method of
    test_captured_pose_step_equals_the_eager_loop, because ray gradients are summed with float atomics (two runs from one state
    differ in the last bits and, left running, take different branches at sample_pdf's bin edges):
    (a) one eager run E is recorded (per step: the state before it, its loss, the update of each parameter group);
        LOCKSTEP_REPEATS more eager passes redo every step from E's recorded state -- their largest distance from E is the spread;
    (b) the captured step replayed from E's recorded states: <= 4x that spread, floor rtol 2e-5, on the loss and on the update of
        every parameter group (relative L2);
    (c) constructing the step leaves parameters, moments and step counts untouched;
    (d) after 8 replays in a row the step counts are 8 on host and device, in both groups;
    (e) step.poses equals learned_poses() evaluated eagerly, before the first replay and after the last."""
    from nerf_shared_amd import optim, render_utils, utils
    s = joint_scene(dev)
    K, images = s["K"], s["images"]
    steps, n, M = 8, N_RAYS, N_IMAGES
    lr_at = lambda k: (5e-4 * (0.8 ** (k / 100)), 2e-3 * (0.8 ** (k / 100)))          # noqa: E731  (field, poses)
    r = render_utils.Renderer(**JOINT_CFG)
    start = utils.perturbed_start_poses(lego44(), 2, 2.0, 0.05, seed=2)[1] @ np.linalg.inv(lego44())   # one small rigid motion
    noisy = np.stack([s["poses"][0]] + [(start @ q).astype(np.float32) for q in s["poses"][1:]])
    batches = []
    for k in range(steps):
        pix_np, p_np = mixed_batch(H20, W20, M, n, seed=100 + k)
        pix, p = torch.from_numpy(pix_np).to(dev), torch.from_numpy(p_np).to(device=dev, dtype=torch.int32)
        batches.append((pix, p, images[p.long(), pix[:, 1], pix[:, 0]].contiguous()))

    def fresh():
        (mc, mf), _ = fog_models(dev, precision)
        lp = utils.LearnedPoses(noisy, frozen=(0,)).to(dev)
        field = list(mc.parameters()) + list(mf.parameters())
        opt = optim.Adam([{"params": field, "lr": lr_at(0)[0]}, {"params": [lp.twist.xi], "lr": lr_at(0)[1]}], betas=(0.9, 0.999))
        return mc, mf, lp, opt

    def groups_flat(opt):
        return [torch.cat([q.detach().flatten() for q in g["params"]]).cpu().double().numpy() for g in opt.param_groups]

    def set_lr(opt, k):
        for g, lr in zip(opt.param_groups, lr_at(k)):
            g["lr"] = lr

    def eager_step(run, k):
        mc, mf, lp, opt = run
        pix, p, tgt = batches[k]
        set_lr(opt, k)
        opt.zero_grad()
        ro, rd = utils.get_rays_indexed(H20, W20, K, lp(), pix, p)
        rgb, _, _, extras = r.render_from_rays(H20, W20, K, 32768, torch.stack([ro, rd], 0), mc, mf, retraw=True)
        loss = utils.img2mse(rgb, tgt) + utils.img2mse(extras["rgb0"], tgt)
        loss.backward()
        opt.step()
        return float(loss.detach())

    def all_params(opt):
        return [q for g in opt.param_groups for q in g["params"]]

    def load(run, state, k):
        """E's state before step k (k >= 1) into a run: parameters, moments, step counts of both groups (host and device)."""
        mc, mf, lp, opt = run
        with torch.no_grad():
            for q, (q0, m0, v0) in zip(all_params(opt), state):
                q.copy_(q0)
                opt.state[q]["exp_avg"].copy_(m0)
                opt.state[q]["exp_avg_sq"].copy_(v0)
        for m in (mc, mf):
            m.weights_changed()
        for gi in opt._together:
            opt._together[gi]["step"] = k
            if opt._device_scalars is not None:
                opt._device_scalars[gi][0].fill_(k)

    run = fresh()                                                              # E: the recorded eager run
    opt = run[3]
    states, losses_e, updates_e = [None], [], []
    for k in range(steps):
        if k > 0:
            states.append([(q.detach().clone(), opt.state[q]["exp_avg"].clone(), opt.state[q]["exp_avg_sq"].clone()) for q in all_params(opt)])
        before = groups_flat(opt)
        losses_e.append(eager_step(run, k))
        updates_e.append([a - b for a, b in zip(groups_flat(opt), before)])
    assert all(np.linalg.norm(u) > 0 for upd in updates_e for u in upd), "degenerate test: a parameter group did not move"
    assert losses_e[0] > 1e-7

    def lockstep(run, one_step):
        worst_l, worst_u = 0.0, [0.0, 0.0]
        for k in range(steps):
            if k > 0:
                load(run, states[k], k)
            before = groups_flat(run[3])
            loss = one_step(k)
            upd = [a - b for a, b in zip(groups_flat(run[3]), before)]
            worst_l = max(worst_l, abs(loss - losses_e[k]) / abs(losses_e[k]))
            for gi in range(2):
                worst_u[gi] = max(worst_u[gi], float(np.linalg.norm(upd[gi] - updates_e[k][gi]) / np.linalg.norm(updates_e[k][gi])))
        return worst_l, worst_u

    repeats = []                                                                                                     # (a)
    for _ in range(LOCKSTEP_REPEATS):
        run = fresh()
        repeats.append(lockstep(run, lambda k: eager_step(run, k)))
    spread_l = max(d[0] for d in repeats)
    spread_u = [max(d[1][gi] for d in repeats) for gi in range(2)]
    del run

    mc, mf, lp, opt = fresh()
    init = [q.detach().clone() for q in all_params(opt)]
    step = utils.CapturedJointStep(r, H20, W20, K, 32768, mc, mf, lp, opt, n)
    assert all(torch.equal(q, q0) for q, q0 in zip(all_params(opt), init))                                           # (c)
    assert len(opt._together) == 2 and all(c["step"] == 0 for c in opt._together.values())
    assert all(int(opt._device_scalars[gi][0]) == 0 for gi in range(2))
    assert all(not st["exp_avg"].any() and not st["exp_avg_sq"].any() for st in opt.state.values())
    with torch.no_grad():
        assert torch.equal(step.poses, lp()) and torch.equal(step.poses[0], torch.from_numpy(noisy[0]).to(dev))      # (e)

    def replay(k):
        set_lr(opt, k)
        return float(step(*batches[k]))

    got = [replay(k) for k in range(steps)]                                     # the free run
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in all_params(opt))
    assert bool((lp.twist.xi.grad[0] == 0).all()) and bool((lp.twist.xi.detach()[0] == 0).all())                     # the frozen view
    assert bool((lp.twist.xi.detach()[1:] != 0).all())
    sd = opt.state_dict()["state"]
    assert all(c["step"] == steps for c in opt._together.values()) and all(int(st["step"]) == steps for st in sd.values())   # (d)
    assert all(int(opt._device_scalars[gi][0]) == steps for gi in range(2))
    with torch.no_grad():
        assert torch.equal(step.poses, lp())                                                                         # (e)
    assert float(step.psnr) > 0 and abs(float(step.loss) - got[-1]) == 0
    print("eager   ", ["%.4e" % v for v in losses_e])
    print("captured", ["%.4e" % v for v in got])
    assert abs(got[0] - losses_e[0]) <= 2e-5 * abs(losses_e[0])                 # same state, deterministic forward

    with torch.no_grad():                                                       # (b): the same captured step, from E's states
        for q, q0 in zip(all_params(opt), init):
            q.copy_(q0)
        for st in opt.state.values():
            st["exp_avg"].zero_(); st["exp_avg_sq"].zero_()
    for m in (mc, mf):
        m.weights_changed()
    for gi in opt._together:
        opt._together[gi]["step"] = 0
        opt._device_scalars[gi][0].fill_(0)
    dist_l, dist_u = lockstep((mc, mf, lp, opt), replay)
    print("eager lockstep repeats (loss, updates):", ["%.2e %s" % (d[0], ["%.2e" % u for u in d[1]]) for d in repeats])
    print("%s lockstep: loss captured vs eager %.3e (spread %.3e); updates field %.3e (%.3e), poses %.3e (%.3e)"
          % (precision, dist_l, spread_l, dist_u[0], spread_u[0], dist_u[1], spread_u[1]))
    assert dist_l <= max(4 * spread_l, 2e-5)
    assert dist_u[0] <= max(4 * spread_u[0], 2e-5)
    assert dist_u[1] <= max(4 * spread_u[1], 2e-5)


def test_captured_joint_step_draws_from_the_image_bank(dev):
    """With sampler=ImageBankSampler the captured body begins with the draw: draw k is the same pixels and colours replayed as
    drawn eagerly by a second sampler of the same seed, construction leaves draw_count where it was, the bank is used in place,
    the first loss equals the eager step's on the same draw, and a sampler of another shape is refused."""
    from nerf_shared_amd import optim, render_utils, utils
    s = joint_scene(dev)
    K, images = s["K"], s["images"]
    r = render_utils.Renderer(**JOINT_CFG)
    (mc, mf), _ = fog_models(dev, "fp32_split")
    lp = utils.LearnedPoses(s["poses"], frozen=(0,)).to(dev)
    field = list(mc.parameters()) + list(mf.parameters())
    opt = optim.Adam([{"params": field, "lr": 5e-4}, {"params": [lp.twist.xi], "lr": 1e-3}], betas=(0.9, 0.999))
    bank = utils.ImageBankSampler(images, N_RAYS, seed=3)
    twin = utils.ImageBankSampler(images, N_RAYS, seed=3)
    assert (bank.M, bank.H, bank.W, bank.n_rays) == (N_IMAGES, H20, W20, N_RAYS) and bank.image.data_ptr() == images.data_ptr()
    bank.reset(2)
    twin.reset(2)
    with pytest.raises(_lib.NerfAmdError, match="sampler draws"):
        utils.CapturedJointStep(r, H20, W20, K, 32768, mc, mf, lp, opt, N_RAYS, sampler=utils.ImageBankSampler(images[:3], N_RAYS))
    with pytest.raises(_lib.NerfAmdError, match="sampler draws"):
        utils.CapturedJointStep(r, H20, W20, K, 32768, mc, mf, lp, opt, 32, sampler=bank)
    # the eager step on draw 2, from the initial state (no optimizer step: the loss alone)
    pix, tgt = (t.clone() for t in twin.draw())
    assert int(pix[:, 1].max()) >= H20 and int(pix[:, 1].max()) < N_IMAGES * H20 and len({tuple(q) for q in pix.tolist()}) == N_RAYS
    assert torch.equal(tgt, images.view(-1, W20, 3)[pix[:, 1].long(), pix[:, 0].long()])
    with torch.no_grad():
        ro, rd = utils.get_rays_indexed(H20, W20, K, lp(), pix)
        rgb, _, _, extras = r.render_from_rays(H20, W20, K, 32768, torch.stack([ro, rd], 0), mc, mf, retraw=True)
        loss_e = float(utils.img2mse(rgb, tgt) + utils.img2mse(extras["rgb0"], tgt))
    twin.reset(2)
    step = utils.CapturedJointStep(r, H20, W20, K, 32768, mc, mf, lp, opt, N_RAYS, sampler=bank)
    assert int(bank.draw_count) == 2
    with pytest.raises(_lib.NerfAmdError, match="without arguments"):
        step(pix, None, tgt)
    for k in range(3):
        loss = float(step())
        pix_e, tgt_e = twin.draw()
        assert torch.equal(step.pixels, pix_e) and torch.equal(step.target, tgt_e), k
        if k == 0:
            assert abs(loss - loss_e) <= 2e-5 * abs(loss_e)
    assert int(bank.draw_count) == 5 == int(twin.draw_count)
    assert bool((lp.twist.xi.detach()[0] == 0).all()) and bool((lp.twist.xi.detach()[1:] != 0).any())
