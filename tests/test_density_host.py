"""CPU tests of the density-query surface: the new C entry points are bound with the header's signatures, the density twin's
arch comes out as documented, CPU tensors are refused, and a model's density twin stays out of copies and pickles."""
import copy
import ctypes
import io
import os
import pickle
import re

import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from nerf_shared_amd import _lib, nerf  # noqa: E402

C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const nerf_amd_arch *": ctypes.POINTER(_lib.Arch),
           "nerf_amd_arch *": ctypes.POINTER(_lib.Arch), "const nerf_amd_model *": ctypes.c_void_p, "const float *": ctypes.c_void_p,
           "float *": ctypes.c_void_p, "void *": ctypes.c_void_p}
NEW = ("nerf_amd_density_arch", "nerf_amd_density", "nerf_amd_density_grad_fused", "nerf_amd_density_grad_workspace",
       "nerf_amd_density_value_grad")


def test_density_symbols_are_bound_with_the_headers_signatures():
    with open(os.path.join(REPO, "include", "nerf_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        m = re.search(r"(int64_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        args = []
        for a in m.group(2).split(","):
            ctype = re.sub(r"\s*\w+\s*$", "", " ".join(a.split()))           # drop the parameter name
            ctype = ctype if ctype.endswith("*") else ctype
            args.append(C_TYPES[ctype.replace(" *", " *")])
        fn = getattr(_lib.lib, name)
        assert name in _lib.EXPORTS
        assert fn.restype is C_TYPES[m.group(1)], name
        assert list(fn.argtypes) == args, (name, fn.argtypes, args)
    assert _lib.lib.nerf_amd_abi_version() == _lib.ABI_VERSION == 7


@pytest.mark.parametrize("multires,multires_views,i_embed", [(10, 4, 0), (15, 6, 0), (10, 4, -1)])
def test_density_arch(multires, multires_views, i_embed):
    lib = _lib.lib
    src = _lib.make_arch(8, 256, 5, [4], True, multires, multires_views, i_embed)
    out = _lib.Arch()
    assert lib.nerf_amd_density_arch(ctypes.byref(src), ctypes.byref(out)) == 0
    assert (out.D, out.W, out.output_ch, out.use_viewdirs, out.multires, out.multires_views, out.i_embed, out.n_skips, out.skips[0]) \
        == (8, 256, 1, 0, multires, 0, i_embed, 1, 4)
    assert (src.output_ch, src.use_viewdirs, src.multires_views) == (5, 1, multires_views)          # the input is not written
    # the twin the Python side builds has this arch
    tw = nerf.NeRF(D=8, W=256, output_ch=5, skips=[4], use_viewdirs=True, multires=multires, multires_views=multires_views,
                   i_embed=i_embed).density_model()
    assert (tw.D, tw.W, tw.output_ch, tw.use_viewdirs, tw.multires, tw.multires_views, tw.i_embed, list(tw.skips)) \
        == (out.D, out.W, out.output_ch, bool(out.use_viewdirs), out.multires, out.multires_views, out.i_embed, [4])
    # a model without view branch: only the head narrows
    nv = _lib.make_arch(4, 128, 7, [2], False, 6, 0, 0)
    assert lib.nerf_amd_density_arch(ctypes.byref(nv), ctypes.byref(out)) == 0
    assert (out.D, out.W, out.output_ch, out.use_viewdirs, out.multires, out.skips[0]) == (4, 128, 1, 0, 6, 2)
    # refusals: null pointers, an arch the library would not build
    assert lib.nerf_amd_density_arch(None, ctypes.byref(out)) == -1
    assert lib.nerf_amd_density_arch(ctypes.byref(src), None) == -1
    bad = _lib.make_arch(8, 256, 4, [7], True, 10, 4, 0)                   # skip on the last layer
    assert lib.nerf_amd_density_arch(ctypes.byref(bad), ctypes.byref(out)) == -1


def test_null_models_and_tuning_key():
    lib = _lib.lib
    assert lib.nerf_amd_density(None, None, 0, None, _lib.PREC_BF16, None) == -1
    assert lib.nerf_amd_density_value_grad(None, None, 0, None, None, None, 0, _lib.PREC_BF16, None) == -1
    assert lib.nerf_amd_density_grad_fused(None, _lib.PREC_BF16) == 0
    assert lib.nerf_amd_density_grad_workspace(None, 10, _lib.PREC_BF16) == -1
    for route in ("two_launch", "auto"):
        nerf.set_density_grad_route(route)
    with pytest.raises(ValueError):
        nerf.set_density_grad_route("both")
    assert lib.nerf_amd_set_tuning(1, 2) == -1


def test_density_queries_refuse_cpu_tensors():
    for m in (nerf.NeRF(use_viewdirs=True), nerf.NeRF(use_viewdirs=False, output_ch=5)):
        with pytest.raises(_lib.NerfAmdError, match="no CPU path"):
            m.get_density(torch.zeros(7, 3))
        with pytest.raises(_lib.NerfAmdError, match="no CPU path"):
            m.get_density(torch.zeros(2, 4, 3))
        with pytest.raises(_lib.NerfAmdError, match="no CPU path"):
            m.density_and_grad(torch.zeros(7, 3))


def test_twin_is_shared_not_copied_and_stays_out_of_copies_and_pickles():
    m = nerf.NeRF(use_viewdirs=True, output_ch=5)
    keys, n_params = list(m.state_dict().keys()), len(list(m.parameters()))
    plain = len(pickle.dumps(m))
    tw = m.density_model()
    assert tw is m.density_model() and tw is not m
    assert all(a.weight is b.weight and a.bias is b.bias
               for a, b in zip(list(m.pts_linears) + [m.alpha_linear], list(tw.pts_linears) + [tw.output_linear]))
    assert not hasattr(tw, "views_linears") and len(list(tw.parameters())) == 18
    assert list(m.state_dict().keys()) == keys and len(list(m.parameters())) == n_params
    assert not any(isinstance(v, nerf.NeRF) for v in m.__dict__.values()) and not any(isinstance(v, nerf.NeRF) for v in m._modules.values())
    # pickles and deep copies hold one model: the same bytes as before the twin existed, and the copy makes its own twin
    assert len(pickle.dumps(m)) == plain
    buf = io.BytesIO()
    torch.save(m, buf)
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert list(c.state_dict().keys()) == keys
        assert c not in nerf._DENSITY_TWINS
        tc = c.density_model()
        assert tc is not tw and tc.pts_linears[0].weight is c.pts_linears[0].weight and tc.pts_linears[0].weight is not m.pts_linears[0].weight
    # the twin follows its model: precision on every call, staleness with weights_changed(), replaced Parameters with a new twin
    m.precision = "fp32_split"
    assert m.density_model().precision == "fp32_split"
    tw._packed_key = ("something",)
    m.weights_changed()
    assert tw._packed_key is None
    m.alpha_linear.weight = torch.nn.Parameter(torch.zeros(1, 256))
    tw2 = m.density_model()
    assert tw2 is not tw and tw2.output_linear.weight is m.alpha_linear.weight
    # a model without view branch is its own twin
    nv = nerf.NeRF(use_viewdirs=False, output_ch=5)
    assert nv.density_model() is nv
    # twins die with their models
    import gc
    n = len(nerf._DENSITY_TWINS)
    del m, tw, tw2
    gc.collect()
    assert len(nerf._DENSITY_TWINS) < n
