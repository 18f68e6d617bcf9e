"""CPU tests of the multi-start pose-estimation surface: the six batched C entry points are bound with the argument counts the
header declares (the ABI stays at 7), utils.CameraTransfBatch keeps B x the demo module's parameters, utils.perturbed_start_poses
makes the hypotheses it documents, and the selection rule (utils.multistart_scores) on a hand-made loss table.  No compute
call reaches a GPU."""
import os
import re

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from nerf_shared_amd import _lib, synth, utils  # noqa: E402

NEW_SYMBOLS = ("nerf_amd_se3_transform_batch", "nerf_amd_se3_transform_batch_backward", "nerf_amd_rays_at_pixels_batch",
               "nerf_amd_rays_at_pixels_batch_backward", "nerf_amd_img2mse_each", "nerf_amd_img2mse_each_backward")


def _declared_argument_counts():
    with open(os.path.join(REPO, "include", "nerf_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    counts = {}
    for name, args in re.findall(r"\b(nerf_amd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        counts[name] = 0 if args.strip() in ("", "void") else len(args.split(","))
    return counts


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_batched_entry_points_are_bound_as_the_header_declares_them(name):
    declared = _declared_argument_counts()
    assert name in _lib.EXPORTS
    assert name in declared, "include/nerf_amd.h does not declare %s" % name
    fn = getattr(_lib.lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == declared[name], (name, len(fn.argtypes or ()), declared[name])


def test_additive_entry_points_leave_the_abi_version_alone():
    assert _lib.lib.nerf_amd_abi_version() == 7 == _lib.ABI_VERSION
    declared = _declared_argument_counts()
    # each batched entry point is its single-pose twin plus the batch arguments
    assert declared["nerf_amd_se3_transform_batch"] == declared["nerf_amd_se3_transform"] + 2              # x_stride, B
    assert declared["nerf_amd_se3_transform_batch_backward"] == declared["nerf_amd_se3_transform_backward"] + 2
    assert declared["nerf_amd_rays_at_pixels_batch"] == declared["nerf_amd_rays_at_pixels"] + 2            # pose stride, B
    assert declared["nerf_amd_rays_at_pixels_batch_backward"] == declared["nerf_amd_rays_at_pixels_backward"]   # + B, - partials
    assert declared["nerf_amd_img2mse_each"] == declared["nerf_amd_img2mse"] + 1                           # + y_stride, B, - partials
    assert declared["nerf_amd_img2mse_each_backward"] == declared["nerf_amd_img2mse_backward"] + 1         # + y_stride, B, - gy


def test_python_limits_are_the_kernels_limits():
    """utils decides between the library and the torch expression with the launchers' own limits (csrc/kernels.h)."""
    with open(os.path.join(REPO, "nerf_shared_amd", "csrc", "kernels.h")) as f:
        m = re.search(r"POSE_BATCH_MAX = (\d+), IMG2MSE_EACH_MAX = (\d+)", f.read())
    assert m and (int(m.group(1)), int(m.group(2))) == (utils.POSE_BATCH_MAX, utils.IMG2MSE_EACH_MAX) == (1024, 16384)


def test_camera_transf_batch_has_b_times_the_demo_modules_parameters():
    torch.manual_seed(11)
    m = utils.CameraTransfBatch(5)
    sd = m.state_dict()
    assert list(sd.keys()) == ["w", "v", "theta"]
    assert tuple(sd["w"].shape) == (5, 3) and tuple(sd["v"].shape) == (5, 3) and tuple(sd["theta"].shape) == (5,)
    assert all(p.requires_grad and p.dtype == torch.float32 for p in m.parameters())
    assert max(float(p.detach().abs().max()) for p in m.parameters()) < 1e-4            # normal(0, 1e-6)
    assert float(m.w.detach().abs().max()) > 0                                         # ... and drawn, not zero
    with pytest.raises(_lib.NerfAmdError):
        m(torch.eye(4))                                                                # no CPU path
    with pytest.raises(_lib.NerfAmdError):
        m(torch.eye(4).repeat(5, 1, 1))
    for bad in (0, 1025):
        with pytest.raises(_lib.NerfAmdError):
            utils.CameraTransfBatch(bad)
    one = m.pose_module(2)
    assert isinstance(one, utils.CameraTransf)
    assert tuple(one.w.shape) == (3,) and tuple(one.v.shape) == (3,) and tuple(one.theta.shape) == ()
    assert torch.equal(one.w, m.w[2]) and torch.equal(one.v, m.v[2]) and torch.equal(one.theta, m.theta[2])
    with torch.no_grad():
        one.w.add_(1.0)                                                                # copies: the batch module does not follow
    assert float(m.w.detach().abs().max()) < 1e-4


def _small_pose():
    """An orthonormal pose with a translation below 1: every fp32 entry of a perturbed pose then carries at most 2^-24 ~ 6e-8
    of rounding, well inside the 1e-6 bounds below."""
    pose = np.eye(4)
    pose[:3, :4] = synth.pose_spherical(35.0).astype(np.float64)
    r = pose[:3, :3]
    u, _, vt = np.linalg.svd(r)
    pose[:3, :3] = u @ vt
    pose[:3, 3] = [0.3, -0.2, 0.5]
    return pose


def test_perturbed_start_poses_are_the_documented_hypotheses():
    pose, n, rot_deg, trans = _small_pose(), 9, 12.5, 0.07
    out = utils.perturbed_start_poses(pose, n, rot_deg, trans, seed=3)
    assert isinstance(out, np.ndarray) and out.shape == (n, 4, 4) and out.dtype == np.float32
    assert np.array_equal(out[0], pose.astype(np.float32))
    axes = []
    for i in range(n):
        R = out[i, :3, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6
        assert np.array_equal(out[i, 3], np.array([0, 0, 0, 1], np.float32))
        if i == 0:
            continue
        D = R @ pose[:3, :3].T                                                 # the left-multiplied rotation
        angle = np.degrees(np.arccos(np.clip((np.trace(D) - 1.0) / 2.0, -1.0, 1.0)))
        assert abs(angle - rot_deg) <= 1e-4, (i, angle)
        t = out[i, :3, 3].astype(np.float64) - D @ pose[:3, 3]
        assert abs(np.linalg.norm(t) - trans) <= 1e-6, (i, np.linalg.norm(t))
        axes.append(np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]]))
    assert np.linalg.matrix_rank(np.stack(axes), tol=1e-3) == 3                # random axes, not one axis eight times
    assert np.array_equal(out, utils.perturbed_start_poses(pose, n, rot_deg, trans, seed=3))
    assert np.array_equal(out, utils.perturbed_start_poses(torch.from_numpy(pose), n, rot_deg, trans, seed=3))
    assert not np.array_equal(out[1:], utils.perturbed_start_poses(pose, n, rot_deg, trans, seed=4)[1:])
    assert utils.perturbed_start_poses(pose, 1, rot_deg, trans).shape == (1, 4, 4)


def test_selection_rule_on_a_hand_made_loss_table():
    nan = float("nan")
    #                  b = 0    1     2    3
    losses = np.array([[9.0, 1.0, 0.1, 5.0],
                       [8.0, 1.0, nan, 5.0],
                       [1.0, 2.0, 0.1, 5.0],
                       [2.0, 2.0, 0.1, nan],
                       [3.0, 2.5, 0.1, nan]], np.float32)
    scores, best = utils.multistart_scores(losses, window=3)                   # rows 2..4: column 2 is clean there
    assert scores.shape == (4,) and best.dim() == 0 and best.dtype == torch.int64
    assert scores.tolist() == [2.0, pytest.approx(6.5 / 3, rel=1e-6), pytest.approx(0.1, rel=1e-6), float("inf")]
    assert int(best) == 2
    scores, best = utils.multistart_scores(losses, window=4)                   # rows 1..4: the NaN of column 2 counts as +inf
    assert scores.tolist() == [3.5, pytest.approx(7.5 / 4, rel=1e-6), float("inf"), float("inf")]
    assert int(best) == 1
    scores, best = utils.multistart_scores(losses, window=10)                  # steps < window: all five rows
    assert scores.tolist() == [pytest.approx(23.0 / 5, rel=1e-6), pytest.approx(8.5 / 5, rel=1e-6), float("inf"), float("inf")]
    assert int(best) == 1
    scores, best = utils.multistart_scores(torch.from_numpy(losses[:, 2:]), window=2)       # a tensor; ties and inf
    assert scores.tolist() == [pytest.approx(0.1, rel=1e-6), float("inf")] and int(best) == 0
    scores, best = utils.multistart_scores(np.full((2, 3), nan, np.float32), window=1)      # nothing finite: still an index
    assert scores.tolist() == [float("inf")] * 3 and 0 <= int(best) < 3
    with pytest.raises(_lib.NerfAmdError):
        utils.multistart_scores(np.zeros((0, 3), np.float32))
    with pytest.raises(_lib.NerfAmdError):
        utils.multistart_scores(np.zeros(3, np.float32))
