"""CPU tests of the joint pose-and-field training surface: the four new C entry points are bound with the argument counts the
header declares (the ABI stays at 7), utils.SE3Twist / utils.LearnedPoses keep the state they document and start at exactly
zero, host pixels and pose indices are checked before anything reaches a device, and utils.ImageBankSampler /
utils.CapturedJointStep refuse what they document.  No compute call reaches a GPU."""
import os
import re

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from nerf_shared_amd import _lib, nerf, optim, synth, utils  # noqa: E402

NEW_SYMBOLS = ("nerf_amd_rays_at_pixels_indexed", "nerf_amd_rays_at_pixels_indexed_backward", "nerf_amd_se3_exp_batch",
               "nerf_amd_se3_exp_batch_backward")


def _declared_argument_counts():
    with open(os.path.join(REPO, "include", "nerf_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    counts = {}
    for name, args in re.findall(r"\b(nerf_amd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        counts[name] = 0 if args.strip() in ("", "void") else len(args.split(","))
    return counts


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_joint_entry_points_are_bound_as_the_header_declares_them(name):
    declared = _declared_argument_counts()
    assert name in _lib.EXPORTS
    assert name in declared, "include/nerf_amd.h does not declare %s" % name
    fn = getattr(_lib.lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == declared[name], (name, len(fn.argtypes or ()), declared[name])


def test_additive_entry_points_leave_the_abi_version_alone():
    assert _lib.lib.nerf_amd_abi_version() == 7 == _lib.ABI_VERSION
    declared = _declared_argument_counts()
    assert declared["nerf_amd_rays_at_pixels_indexed"] == declared["nerf_amd_rays_at_pixels_batch"] + 1            # + pose_index
    assert declared["nerf_amd_rays_at_pixels_indexed_backward"] == declared["nerf_amd_rays_at_pixels_batch_backward"] + 1
    assert declared["nerf_amd_se3_exp_batch"] == declared["nerf_amd_se3_transform_batch"] - 2                      # xi for w, v, theta
    assert declared["nerf_amd_se3_exp_batch_backward"] == declared["nerf_amd_se3_transform_batch_backward"] - 4


def test_the_header_states_the_series_threshold_the_kernel_uses():
    with open(os.path.join(REPO, "nerf_shared_amd", "csrc", "kernels.h")) as f:
        text = f.read()
    th2 = float(re.search(r"SE3_SERIES_TH2 = ([0-9.e+-]+);", text).group(1))
    terms = int(re.search(r"SE3_SERIES_TERMS = (\d+);", text).group(1))
    assert (th2, terms) == (1e-2, 5)
    with open(os.path.join(REPO, "include", "nerf_amd.h")) as f:
        header = f.read()
    assert "th^2 < 1e-2" in header and "FIVE" in header


def test_se3_twist_starts_at_exactly_zero_and_has_no_cpu_path():
    m = utils.SE3Twist(5)
    sd = m.state_dict()
    assert list(sd.keys()) == ["xi"] and tuple(sd["xi"].shape) == (5, 6) and sd["xi"].dtype == torch.float32
    assert m.xi.requires_grad and not m.xi.detach().any() and m.n_poses == 5
    with pytest.raises(_lib.NerfAmdError, match="no CPU path"):
        m(torch.eye(4))
    with pytest.raises(_lib.NerfAmdError, match="no CPU path"):
        m(torch.eye(4).repeat(5, 1, 1))
    for bad_shape in ((3, 4), (4, 4, 4), (6, 4, 4)):
        with pytest.raises(_lib.NerfAmdError, match="takes a"):
            m(torch.zeros(bad_shape))
    for bad in (0, 1025):
        with pytest.raises(_lib.NerfAmdError):
            utils.SE3Twist(bad)
    assert utils.SE3Twist(1024).xi.shape == (1024, 6)


def _poses(M):
    return np.stack([np.concatenate([synth.pose_spherical(30.0 * i).astype(np.float32)[:3], [[0, 0, 0, 1]]], 0) for i in range(M)]).astype(np.float32)


def test_learned_poses_hold_the_given_poses_and_a_zero_twist():
    given = _poses(4)
    lp = utils.LearnedPoses(given, frozen=(2, 0, 2))
    sd = lp.state_dict()
    assert list(sd.keys()) == ["poses", "twist.xi"]
    assert tuple(sd["poses"].shape) == (4, 4, 4) and tuple(sd["twist.xi"].shape) == (4, 6)
    assert torch.equal(sd["poses"], torch.from_numpy(given)) and not sd["twist.xi"].any()
    assert lp.frozen == (0, 2) and lp.n_poses == 4 and lp.free.flatten().tolist() == [0.0, 1.0, 0.0, 1.0]
    assert [n for n, _ in lp.named_parameters()] == ["twist.xi"]
    with pytest.raises(_lib.NerfAmdError, match="no CPU path"):
        lp()
    three = utils.LearnedPoses(torch.from_numpy(given[:, :3]))                            # [M, 3, 4]: the last row is appended
    assert torch.equal(three.poses, torch.from_numpy(given)) and three.frozen == ()
    other = utils.LearnedPoses(np.zeros((4, 4, 4), np.float32))
    other.load_state_dict(sd)
    assert torch.equal(other.poses, lp.poses)
    for bad in (np.zeros((0, 4, 4)), np.zeros((4, 4)), np.zeros((2, 4, 3)), np.zeros((1025, 4, 4), np.float32)):
        with pytest.raises(_lib.NerfAmdError, match="LearnedPoses takes"):
            utils.LearnedPoses(bad)
    for bad in ((4,), (-1,), (0, 7)):
        with pytest.raises(_lib.NerfAmdError, match="frozen"):
            utils.LearnedPoses(given, frozen=bad)


def test_host_pixels_and_pose_indices_are_checked_before_the_device():
    H, W, M = 5, 7, 3
    K = synth.lego_intrinsics(H, W)
    c2w = torch.from_numpy(_poses(M))
    for bad in ([[W, 0]], [[0, H]], [[-1, 3]], torch.tensor([[3, 3], [0, H]])):
        with pytest.raises(_lib.NerfAmdError, match="outside"):
            utils.get_rays_indexed(H, W, K, c2w, bad, [0] * len(bad))
    for bad in ([[W, 0]], [[0, M * H]], [[0, -1]]):                                         # stacked rows: y in [0, M H)
        with pytest.raises(_lib.NerfAmdError, match="outside"):
            utils.get_rays_indexed(H, W, K, c2w, bad)
    for bad in ([M], [-1], torch.tensor([0]).expand(1) + M, np.array([2 ** 31 - 1])):
        with pytest.raises(_lib.NerfAmdError, match=r"outside \[0, 3\)"):
            utils.get_rays_indexed(H, W, K, c2w, [[1, 1]], bad)
    with pytest.raises(_lib.NerfAmdError, match="one per pixel"):
        utils.get_rays_indexed(H, W, K, c2w, [[1, 1], [2, 2]], [0])
    with pytest.raises(_lib.NerfAmdError, match="one per pixel"):
        utils.get_rays_indexed(H, W, K, c2w, [[1, 1]], [0.0])
    with pytest.raises(_lib.NerfAmdError, match="ROCm tensor"):                            # valid host inputs: only the device is missing
        utils.get_rays_indexed(H, W, K, c2w, [[6, 4], [0, 0]], [2, 0])
    with pytest.raises(_lib.NerfAmdError, match="ROCm tensor"):
        utils.get_rays_indexed(H, W, K, c2w, [[6, M * H - 1]])
    for bad in (c2w[0], torch.zeros(0, 4, 4), torch.zeros(2, 4, 3), torch.zeros(1025, 3, 4), _poses(2)):
        with pytest.raises(_lib.NerfAmdError, match="pose table"):
            utils.get_rays_indexed(H, W, K, bad, [[0, 0]], [0])


def test_image_bank_sampler_refusals():
    for bad in (torch.zeros(4, 5, 3), torch.zeros(2, 4, 5, 2), torch.zeros(0, 4, 5, 3), np.zeros((2, 4, 5))):
        with pytest.raises(_lib.NerfAmdError, match="image bank"):
            utils.ImageBankSampler(bad, 4)
    big = torch.zeros(1, 1, 1, 3).expand(2, 32768, 32768, 3)                               # 2^31 pixels, no memory behind them
    with pytest.raises(_lib.NerfAmdError, match="2\\^31 - 1"):
        utils.ImageBankSampler(big, 4)
    with pytest.raises(_lib.NerfAmdError):                                                  # a host bank and no device to put it on
        utils.ImageBankSampler(torch.zeros(2, 4, 5, 3), 4, device="cpu")


ARCH = dict(D=2, W=32, output_ch=5, skips=[1], use_viewdirs=True, multires=10, multires_views=4)


def test_captured_joint_step_refusals_that_need_no_device():
    H = W = 20
    K = synth.lego_intrinsics(H, W)
    mc, mf = nerf.NeRF(**ARCH), nerf.NeRF(**ARCH)
    lp = utils.LearnedPoses(_poses(3))
    field = list(mc.parameters()) + list(mf.parameters())
    groups = lambda: [{"params": field, "lr": 5e-4}, {"params": [lp.twist.xi], "lr": 1e-3}]          # noqa: E731
    build = lambda opt, poses=lp, **kw: utils.CapturedJointStep(None, H, W, K, 1024, mc, mf, poses, opt, 64, **kw)   # noqa: E731
    with pytest.raises(_lib.NerfAmdError, match="optim.Adam"):
        build(torch.optim.Adam(groups()))
    with pytest.raises(_lib.NerfAmdError, match="LearnedPoses"):
        build(optim.Adam(groups()), poses=utils.SE3Twist(3))
    with pytest.raises(_lib.NerfAmdError, match="must hold learned_poses.twist.xi"):
        build(optim.Adam(field, lr=5e-4))
    with pytest.raises(_lib.NerfAmdError, match="neither field parameters"):
        build(optim.Adam(groups() + [{"params": [torch.nn.Parameter(torch.zeros(3))]}]))
    with pytest.raises(_lib.NerfAmdError, match="neither field parameters"):               # another module's xi is foreign too
        build(optim.Adam(groups() + [{"params": [utils.SE3Twist(3).xi]}]))
    with pytest.raises(_lib.NerfAmdError, match="ImageBankSampler"):
        build(optim.Adam(groups()), sampler=object())
    with pytest.raises(_lib.NerfAmdError, match="no CPU path"):                            # all accepted: only the device is missing
        build(optim.Adam(groups()))
    mf.requires_grad_(False)
    with pytest.raises(_lib.NerfAmdError, match="CapturedMultiPoseStep"):
        build(optim.Adam(groups()))
    mc.requires_grad_(False)
    with pytest.raises(_lib.NerfAmdError, match="CapturedMultiPoseStep"):
        build(optim.Adam([lp.twist.xi], lr=1e-3))
