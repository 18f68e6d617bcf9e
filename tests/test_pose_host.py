"""CPU tests of the pose-estimation surface: the new C entry points are bound with the argument counts the header declares,
and utils.CameraTransf keeps the demo module's parameters (demo_est_rel_pose.py:36-66).  No compute call reaches a GPU."""
import os
import re

import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from nerf_shared_amd import _lib, utils  # noqa: E402

NEW_SYMBOLS = ("nerf_amd_rays_at_pixels", "nerf_amd_rays_at_pixels_backward", "nerf_amd_se3_transform",
               "nerf_amd_se3_transform_backward", "nerf_amd_field_backward_inputs")


def _declared_argument_counts():
    with open(os.path.join(REPO, "include", "nerf_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    counts = {}
    for name, args in re.findall(r"\b(nerf_amd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        counts[name] = 0 if args.strip() in ("", "void") else len(args.split(","))
    return counts


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_new_entry_points_are_bound_as_the_header_declares_them(name):
    declared = _declared_argument_counts()
    assert name in _lib.EXPORTS
    assert name in declared, "include/nerf_amd.h does not declare %s" % name
    fn = getattr(_lib.lib, name)
    assert fn.argtypes is not None and len(fn.argtypes) == declared[name], (name, len(fn.argtypes or ()), declared[name])


def test_header_parser_agrees_with_a_known_binding():
    """The counting above on functions that existed before: it reads the header the way the bindings were written."""
    declared = _declared_argument_counts()
    for name in ("nerf_amd_field_backward", "nerf_amd_get_rays_backward", "nerf_amd_make_rays", "nerf_amd_abi_version"):
        assert len(getattr(_lib.lib, name).argtypes) == declared[name], name
    assert declared["nerf_amd_field_backward_inputs"] == declared["nerf_amd_field_backward"] - 3      # no weight / bias tables, no count


def test_camera_transf_has_the_demo_modules_parameters():
    m = utils.CameraTransf()
    sd = m.state_dict()
    assert list(sd.keys()) == ["w", "v", "theta"]
    assert tuple(sd["w"].shape) == (3,) and tuple(sd["v"].shape) == (3,) and tuple(sd["theta"].shape) == ()
    assert all(p.requires_grad and p.dtype == torch.float32 for p in m.parameters())
    assert max(float(p.detach().abs().max()) for p in m.parameters()) < 1e-4            # normal(0, 1e-6)
    with pytest.raises(_lib.NerfAmdError):
        m(torch.eye(4))                                                        # no CPU path


def test_host_pixels_outside_the_image_are_refused_before_any_device_work():
    with pytest.raises(_lib.NerfAmdError):
        utils._device_pixels([[0, 0], [7, 2]], 5, 7, torch.device("cpu"))      # x = W
    with pytest.raises(_lib.NerfAmdError):
        utils._device_pixels(torch.tensor([[0, 5]]), 5, 7, torch.device("cpu"))    # y = H
    with pytest.raises(_lib.NerfAmdError):
        utils._device_pixels([[-1, 0]], 5, 7, torch.device("cpu"))
    with pytest.raises(_lib.NerfAmdError):
        utils._device_pixels([[0.5, 0.0]], 5, 7, torch.device("cpu"))          # not integers
    ok = utils._device_pixels([[6, 4], [0, 0]], 5, 7, torch.device("cpu"))
    assert ok.dtype == torch.int32 and ok.tolist() == [[6, 4], [0, 0]]
