"""CPU tests of the ray bounds (include/nerf_amd.h, nerf_amd_occupancy_ray_bounds): the entry point is bound with the header's
signature and refuses bad grids and arguments before any launch, occupancy.RayBounds refuses bad probes / pad,
Renderer.ray_bounds defaults to None -- and the definition, on the mirror (tests/ray_bounds_mirror.py), keeps what the header
promises: for a convex live set and pad >= 1 no sample that looks up live is left out, the inputs of
tests/test_gpu_ray_bounds.py exercise narrowing and misses, and a scalar restatement of the header's text agrees with the
vectorised mirror bit for bit."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

os.environ.setdefault("NERF_AMD_QUIET", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import occupancy_mirror as M  # noqa: E402
import ray_bounds_mirror as B  # noqa: E402
import test_occupancy_host as H  # noqa: E402
import test_train_cull_host as C  # noqa: E402
from nerf_shared_amd import _lib, occupancy, render_utils  # noqa: E402

lib = _lib.lib
NAME = "nerf_amd_occupancy_ray_bounds"


def test_the_symbol_is_bound_with_the_headers_signature():
    with open(os.path.join(REPO, "include", "nerf_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"(int64_t|int)\s+%s\s*\(([^)]*)\)\s*;" % NAME, text)
    assert m, NAME
    args = [H.C_TYPES[re.sub(r"\s*\w+\s*$", "", " ".join(a.split()))] for a in m.group(2).split(",")]      # drop the parameter names
    fn = getattr(lib, NAME)
    assert NAME in _lib.EXPORTS
    assert fn.restype is H.C_TYPES[m.group(1)]
    assert list(fn.argtypes) == args, (fn.argtypes, args)
    assert lib.nerf_amd_abi_version() == _lib.ABI_VERSION == 7          # additive: the version stays


def _call(grid=None, rays=1, ray_ch=8, R=1, probes=64, pad=1, rays_out=2, bounds=3, span=4):
    """Pointers are never dereferenced on the host: every call of this file is refused before a launch (or has R == 0)."""
    g = H._grid() if grid is None else grid
    return lib.nerf_amd_occupancy_ray_bounds(ctypes.byref(g), rays, ray_ch, R, probes, pad, rays_out, bounds, span, None)


@pytest.mark.parametrize("bad", [dict(probes=0), dict(probes=63), dict(probes=96), dict(probes=8192), dict(probes=32), dict(probes=-64),
                                 dict(pad=-1), dict(probes=64, pad=65), dict(probes=4096, pad=4097),
                                 dict(rays_out=None, bounds=None, span=None), dict(rays=8, rays_out=8), dict(ray_ch=9),
                                 dict(R=-1), dict(R=1 << 31), dict(rays=None)])
def test_bad_arguments_are_refused_before_any_launch(bad):
    assert _call(**bad) == -1
    assert b"ray_bounds" in lib.nerf_amd_last_error()


@pytest.mark.parametrize("bad", [dict(n=(0, 4, 4)), dict(n=(4, 1025, 4)), dict(lo=(1, -1, -1)), dict(hi=(float("inf"), 1, 1)),
                                 dict(lo=(float("nan"), -1, -1)), dict(outside=2), dict(words=None)])
def test_bad_grids_are_refused_before_any_launch(bad):
    assert _call(grid=H._grid(**bad)) == -1
    assert b"grid" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_occupancy_ray_bounds(None, 1, 8, 1, 64, 1, 2, 3, 4, None) == -1


def test_no_rays_is_ok_and_launches_nothing():
    assert _call(R=0, rays=None) == 0
    assert _call(R=0, rays=None, pad=64, probes=64, rays_out=None, span=None) == 0          # pad == P and one output are fine
    for p in (64, 128, 256, 512, 1024, 2048, 4096):
        assert _call(R=0, rays=None, probes=p) == 0


def test_ray_bounds_refuses_bad_probes_and_pad_and_the_renderer_defaults_to_none():
    g = occupancy.OccupancyGrid([[-1, -1, -1], [1, 1, 1]], 4, device="cuda:0")          # building either touches no device
    for bad in (0, 63, 96, 8192, 32, -64, 256.0, "256", None, True):
        with pytest.raises(ValueError, match="probes"):
            occupancy.RayBounds(g, probes=bad)
    for bad in (-1, 257, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="pad"):
            occupancy.RayBounds(g, probes=256, pad=bad)
    with pytest.raises(ValueError, match="pad"):
        occupancy.RayBounds(g, probes=64, pad=65)
    with pytest.raises(TypeError):
        occupancy.RayBounds(None)
    rb = occupancy.RayBounds(g)
    assert (rb.grid, rb.probes, rb.pad) == (g, 256, 1)
    rb = occupancy.RayBounds(g, 64, 64)
    assert (rb.probes, rb.pad) == (64, 64)
    assert g._words is None                                            # nothing above touched a device
    assert render_utils.Renderer.ray_bounds is None
    r = render_utils.Renderer(perturb=0.0)
    assert r.ray_bounds is None and "ray_bounds" not in r.__dict__ and "ray_bounds" not in r.state_dict()
    assert r.occupancy is None and r.train_occupancy is None


# ------------------------------------------------------------------------------------------------ convex containment
BOX_LO, BOX_HI = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)
BLOCKS = (((4, 4, 4), (1, 3)), ((8, 6, 5), (2, 4)), ((16, 16, 16), (5, 11)))


def block_mask(n, blk):
    mask = np.zeros(n, bool)
    mask[blk[0]:blk[1], blk[0]:blk[1], blk[0]:blk[1]] = True
    return mask


def sphere_rays(rng, R):
    """R rays from the sphere of radius 4 toward points of [-1.6, 1.6]^3, |d| in [0.7, 1.4], near 2, far 6."""
    o = rng.normal(size=(R, 3))
    o = 4.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-1.6, 1.6, size=(R, 3)) - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.7, 1.4, size=(R, 1))
    return np.concatenate([o, d, np.full((R, 1), 2.0), np.full((R, 1), 6.0)], 1).astype(np.float32)


def convex_case(i, R=2000):
    """(rays, mask, resolution) of the i-th solid block; the rays of block i are the i-th draw of one seeded generator."""
    rng = np.random.default_rng(0)
    for _ in range(i):
        sphere_rays(rng, R)
    n, blk = BLOCKS[i]
    return sphere_rays(rng, R), block_mask(n, blk), n


@pytest.mark.parametrize("i", range(len(BLOCKS)))
def test_convex_live_set_with_pad_loses_no_live_sample(i):
    rays, mask, n = convex_case(i)
    near, far = rays[:, 6], rays[:, 7]
    dense = {}
    for S in (64, 192):
        z = B.ladder(rays, S)
        dense[S] = z, M.live(M.lookup(M.ray_points(rays, z).reshape(-1, 3), BOX_LO, BOX_HI, n), mask, False).reshape(-1, S)
    live = outside = narrowed = misses = 0
    for P in (64, 256, 1024):
        for pad in (1, 2):
            _, b, span = B.ray_bounds(rays, mask, BOX_LO, BOX_HI, False, P, pad)
            assert np.all(near <= b[:, 0]) and np.all(b[:, 0] <= b[:, 1]) and np.all(b[:, 1] <= far)
            hit = span[:, 0] >= 0
            assert np.array_equal(b[~hit], rays[~hit, 6:8])
            narrowed += int((hit & ((b[:, 0] > near) | (b[:, 1] < far))).sum())
            misses += int((~hit).sum())
            for S, (z, on) in dense.items():
                live += int(on.sum())
                outside += int((on & ((z < b[:, :1]) | (z > b[:, 1:]))).sum())
    print("block %s of %s: %d live dense samples, %d outside the bounds; %d narrowed rays, %d misses" % (BLOCKS[i][1], n, live, outside,
                                                                                                     narrowed, misses))
    assert live > 50000 and narrowed > 1000                            # the case is not vacuous
    assert outside == 0


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
def test_gpu_test_inputs_exercise_narrowing_and_misses():
    rays, mask = C.batch_np(11), C.half_live_mask()
    near, far = rays[:, 6], rays[:, 7]
    _, b, span = B.ray_bounds(rays, mask, C.LO, C.HI, False, 64, 1)                      # 'empty'
    both = int(((b[:, 0] > near) & (b[:, 1] < far)).sum())
    print("'empty': %d rays narrowed at both ends, %d misses" % (both, int((span[:, 0] < 0).sum())))
    assert both >= 35 and (span[:, 0] < 0).sum() >= 1
    _, b, span = B.ray_bounds(rays, mask, C.LO, C.HI, True, 64, 1)                       # 'live'
    either = int(((b[:, 0] > near) | (b[:, 1] < far)).sum())
    print("'live': %d rays narrowed, %d misses" % (either, int((span[:, 0] < 0).sum())))
    assert either >= 10 and (span[:, 0] >= 0).all()


# ------------------------------------------------------------------------------------------------ the header's text, by hand
def _bounds_by_hand(ray, mask, lo, hi, outside_live, P, pad):
    """The header's definition in scalar float32 operations: plain loops, nothing vectorised, nothing shared with the mirror."""
    f = np.float32
    n = mask.shape
    lo32, hi32 = [f(v) for v in lo], [f(v) for v in hi]
    scale = [f(n[a] / (float(hi32[a]) - float(lo32[a]))) for a in range(3)]              # formed in double, rounded once
    near, far = f(ray[6]), f(ray[7])
    w = f(far - near)
    first = last = -1
    for k in range(P):
        u = f((k + 0.5) / P)
        t = f(near + f(w * u))
        idx, inside = [], True
        for a in range(3):
            p = f(f(ray[a]) + f(f(ray[3 + a]) * t))
            ta = f(f(p - lo32[a]) * scale[a])
            if not (ta >= 0 and ta < f(n[a])):                         # false for NaN
                inside = False
                break
            idx.append(int(math.floor(float(ta))))
        on = bool(mask[idx[0], idx[1], idx[2]]) if inside else outside_live
        if on:
            first = k if first < 0 else first
            last = k
    if first < 0:
        return (near, far), (-1, -1)
    k0, k1 = max(first - pad, 0), min(last + pad, P - 1)
    near2 = near if k0 == 0 else f(near + f(w * f(k0 / P)))
    far2 = far if k1 == P - 1 else f(near + f(w * f((k1 + 1) / P)))
    return (near2, far2), (first, last)


@pytest.mark.parametrize("outside_live", [False, True])
def test_a_scalar_restatement_of_the_header_agrees_with_the_mirror(outside_live):
    rays, mask = C.batch_np(11)[[0, 17, 33, 52, 69]], C.half_live_mask()
    for pad in (0, 1, 64):
        out, b, span = B.ray_bounds(rays, mask, C.LO, C.HI, outside_live, 64, pad)
        for r in range(rays.shape[0]):
            with np.errstate(invalid="ignore"):
                (n2, f2), sp = _bounds_by_hand(rays[r], mask, C.LO, C.HI, outside_live, 64, pad)
            assert np.float32(n2).view(np.uint32) == b[r, 0].view(np.uint32) and np.float32(f2).view(np.uint32) == b[r, 1].view(np.uint32)
            assert sp == tuple(span[r])
        assert np.array_equal(out[:, 6:8].view(np.uint32), b.view(np.uint32))
        keep = [c for c in range(11) if c not in (6, 7)]
        assert np.array_equal(out[:, keep].view(np.uint32), rays[:, keep].view(np.uint32))


def test_the_training_demo_refuses_a_bad_pad_before_any_step():
    import sys
    from types import SimpleNamespace
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import train_demo
    r = SimpleNamespace(train_occupancy=1, ray_bounds=1)
    for probes, pad, what in ((256, 257, "pad"), (256, -1, "pad"), (96, 1, "probes")):
        with pytest.raises(ValueError, match=what):
            train_demo.train_culled(r, None, None, None, 8, 8, None, 64, 16, None, None, 0, 10, train_demo.SPHERE_BOX, 4,
                                    ray_bounds_probes=probes, ray_bounds_pad=pad)
