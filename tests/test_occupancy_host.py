"""CPU tests of the occupancy-grid surface: the new C entry points are bound with the header's signatures, the workspace
function agrees with a hand count, grids the library would not take are refused on the host, CPU tensors and bad
resolutions are refused, Renderer.occupancy defaults to None -- and the mirror (tests/occupancy_mirror.py) keeps its own
promises: its jittered samples look up to their own cells, its dilation is max_pool3d, and the inputs of the exact culling
test of tests/test_gpu_occupancy.py cull at least a quarter of their samples on the CPU oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import occupancy_mirror as M  # noqa: E402
from nerf_shared_amd import _lib, occupancy, render_utils, synth  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402

lib = _lib.lib
GRID_P = ctypes.POINTER(_lib.OccupancyGridC)
C_TYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float,
           "const nerf_amd_occupancy_grid *": GRID_P, "const nerf_amd_model *": ctypes.c_void_p,
           "const nerf_amd_render_cfg *": ctypes.POINTER(_lib.RenderCfg), "const nerf_amd_render_io *": ctypes.POINTER(_lib.RenderIO),
           "const float *": ctypes.c_void_p, "float *": ctypes.c_void_p, "const int32_t *": ctypes.c_void_p, "int32_t *": ctypes.c_void_p,
           "uint8_t *": ctypes.c_void_p, "void *": ctypes.c_void_p, "int64_t *": None}
NEW = ("nerf_amd_occupancy_query", "nerf_amd_occupancy_sample_points", "nerf_amd_occupancy_mark", "nerf_amd_occupancy_dilate",
       "nerf_amd_occupancy_cull", "nerf_amd_occupancy_expand", "nerf_amd_field_points", "nerf_amd_render_rays_culled_workspace",
       "nerf_amd_render_rays_culled")
# int64_t * is a DEVICE pointer in the kernels' entry points and a HOST array in the render entry point
INT64_P = {"nerf_amd_occupancy_cull": ctypes.c_void_p, "nerf_amd_render_rays_culled": ctypes.POINTER(ctypes.c_int64)}


def test_new_symbols_are_bound_with_the_headers_signatures():
    with open(os.path.join(REPO, "include", "nerf_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        m = re.search(r"(int64_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        args = []
        for a in m.group(2).split(","):
            ctype = re.sub(r"\s*\w+\s*$", "", " ".join(a.split()))           # drop the parameter name
            args.append(INT64_P[name] if ctype == "int64_t *" else C_TYPES[ctype])
        fn = getattr(lib, name)
        assert name in _lib.EXPORTS
        assert fn.restype is C_TYPES[m.group(1)], name
        assert list(fn.argtypes) == args, (name, fn.argtypes, args)
    assert lib.nerf_amd_abi_version() == _lib.ABI_VERSION == 7          # additive: the version stays
    # the grid struct as the header lays it out: pointer, 3 + 3 floats, 3 + 1 int32
    assert ctypes.sizeof(_lib.OccupancyGridC) == 8 + 4 * (3 + 3 + 3 + 1)
    assert (_lib.OccupancyGridC.lo.offset, _lib.OccupancyGridC.hi.offset, _lib.OccupancyGridC.n.offset, _lib.OccupancyGridC.outside.offset) \
        == (8, 20, 32, 44)


def _cfg(Nc, Ni):
    cfg = _lib.RenderCfg()
    cfg.N_samples, cfg.N_importance, cfg.precision = Nc, Ni, _lib.PREC_BF16
    return cfg


@pytest.mark.parametrize("R,Nc,Ni,ch", [(300, 64, 128, 4), (1, 3, 1, 5), (1025, 64, 0, 4), (0, 64, 128, 4)])
def test_culled_workspace_is_the_dense_one_plus_one_pass_of_compaction_scratch(R, Nc, Ni, ch):
    up = lambda b: (b + 255) // 256 * 256          # noqa: E731  (every piece is 256-byte aligned)
    P = R * (Nc + Ni)                              # the larger pass; the coarse pass reuses its scratch
    extra = up(4 * P) + up(4 * ((P + 255) // 256)) + up(12 * P) + up(12 * P) + up(4 * ch * P) + up(8)
    #       rank        block counts                 pts_live     vd_live      raw_live          count
    cfg = _cfg(Nc, Ni)
    dense = lib.nerf_amd_render_rays_workspace(cfg, R, ch)
    assert lib.nerf_amd_render_rays_culled_workspace(cfg, R, ch) == dense + extra
    assert lib.nerf_amd_render_rays_culled_workspace(None, R, ch) == -1
    assert lib.nerf_amd_render_rays_culled_workspace(cfg, -1, ch) == -1


def _grid(lo=(-1, -1, -1), hi=(1, 1, 1), n=(4, 4, 4), outside=0, words=1):
    g = _lib.OccupancyGridC()
    g.words = words          # never dereferenced on the host: every call below is refused before a launch
    for a in range(3):
        g.lo[a], g.hi[a], g.n[a] = lo[a], hi[a], n[a]
    g.outside = outside
    return g


@pytest.mark.parametrize("bad", [dict(n=(0, 4, 4)), dict(n=(4, 1025, 4)), dict(n=(4, 4, -1)), dict(lo=(1, -1, -1)), dict(hi=(1, 1, -1)),
                                 dict(hi=(float("inf"), 1, 1)), dict(lo=(float("nan"), -1, -1)), dict(outside=2), dict(words=None)])
def test_bad_grids_are_refused_before_any_launch(bad):
    g = _grid(**bad)
    assert lib.nerf_amd_occupancy_query(ctypes.byref(g), 1, 1, 1, None, None) == -1
    assert lib.nerf_amd_occupancy_cull(ctypes.byref(g), 1, 8, 1, 1, 1, 1, 1, 1, None, 1, None) == -1
    assert lib.nerf_amd_render_rays_culled(_cfg(64, 0), None, None, None, 0, ctypes.byref(g), None, None) == -1
    if "words" not in bad:
        assert lib.nerf_amd_occupancy_sample_points(ctypes.byref(g), 0, 1, 1, 0, 1, None) == -1
    assert lib.nerf_amd_last_error()


def test_bad_arguments_are_refused_before_any_launch():
    g = _grid()
    assert lib.nerf_amd_occupancy_query(None, 1, 1, 1, None, None) == -1
    assert lib.nerf_amd_occupancy_sample_points(ctypes.byref(g), 0, 65, 1, 0, 1, None) == -1           # past the last cell
    assert lib.nerf_amd_occupancy_sample_points(ctypes.byref(g), 0, 1, 0, 0, 1, None) == -1            # K < 1
    far = _grid(lo=(1000, -1, -1), hi=(1001, 1, 1), n=(1024, 4, 4))                                    # 1001 * 1024 / 1 > 4096
    assert lib.nerf_amd_occupancy_sample_points(ctypes.byref(far), 0, 1, 1, 0, 1, None) == -1
    assert b"4096" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_occupancy_mark(1, 16, 64, 4, 0.0, 0, 1, None) == -1                            # c0 not a multiple of 32
    assert lib.nerf_amd_occupancy_mark(None, 0, 64, 4, 0.0, 0, 1, None) == -1
    assert lib.nerf_amd_occupancy_dilate(1, 4, 4, 4, 1, 1, None) == -1                                 # in place
    assert lib.nerf_amd_occupancy_dilate(1, 4, 4, 0, 1, 2, None) == -1
    assert lib.nerf_amd_occupancy_dilate(1, 4, 4, 4, -1, 2, None) == -1
    assert lib.nerf_amd_occupancy_cull(ctypes.byref(g), 1, 9, 1, 1, 1, 1, 1, 1, None, 1, None) == -1   # ray_ch
    assert lib.nerf_amd_occupancy_cull(ctypes.byref(g), 1, 8, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1      # vd_live without view columns
    assert lib.nerf_amd_occupancy_cull(ctypes.byref(g), 1, 8, 1, 1 << 26, 32, 1, 1, 1, None, 1, None) == -1      # R S = 2^31
    assert lib.nerf_amd_occupancy_expand(None, None, 5, 4, None, None) == -1
    assert lib.nerf_amd_occupancy_expand(None, None, 0, 4, None, None) == 0
    assert lib.nerf_amd_field_points(None, None, None, 0, None, _lib.PREC_BF16, None) == -1
    noisy = _cfg(64, 0)
    noisy.use_noise = 1
    assert lib.nerf_amd_render_rays_culled(noisy, None, None, None, 0, ctypes.byref(g), None, None) == -1
    assert b"noise" in lib.nerf_amd_last_error()


def test_grid_constructor_refuses_bad_resolutions_boxes_and_cpu():
    box = [[-1, -2, -3], [1, 2, 3]]
    for res in (0, 1025, (4, 4), (4, 0, 4), (4, 4, 2000), 3.5, (4, 4, 4.0)):
        with pytest.raises(ValueError, match="resolution"):
            occupancy.OccupancyGrid(box, res, device="cuda:0")
    for bad in ([[-1, -1, -1], [1, 1, -1]], [[0, 0, 0], [1, 1, float("inf")]], [0, 1, 2]):
        with pytest.raises(ValueError, match="aabb"):
            occupancy.OccupancyGrid(bad, 4, device="cuda:0")
    with pytest.raises(ValueError, match="outside"):
        occupancy.OccupancyGrid(box, 4, outside="dead", device="cuda:0")
    with pytest.raises(_lib.NerfAmdError, match="no CPU path"):
        occupancy.OccupancyGrid(box, 4, device="cpu")
    g = occupancy.OccupancyGrid(box, (5, 7, 33), outside="empty", device="cuda:0")          # building a grid touches no device
    assert (g.n_cells, g.n_words, g.resolution) == (1155, 37, (5, 7, 33))
    c = g._c(words=False)
    assert (list(c.lo), list(c.hi), list(c.n), c.outside) == ([-1, -2, -3], [1, 2, 3], [5, 7, 33], _lib.OCC_OUTSIDE_EMPTY)
    for call in (g.query, g.cell_index):
        with pytest.raises(_lib.NerfAmdError, match="no CPU path"):
            call(torch.zeros(7, 3))
    with pytest.raises(_lib.NerfAmdError, match="no CPU path"):
        g.set_mask(torch.ones(5, 7, 33, dtype=torch.bool))
    with pytest.raises(ValueError):
        g.sample_points(0, 1156)
    with pytest.raises(ValueError):
        g.fill_from_density([])


def test_renderer_occupancy_defaults_to_none():
    assert render_utils.Renderer.occupancy is None and render_utils.Renderer.last_cull is None
    r = render_utils.Renderer(perturb=0.0)
    assert r.occupancy is None and "occupancy" not in r.__dict__ and "occupancy" not in r.state_dict()
    import inspect
    assert list(inspect.signature(render_utils.Renderer.__init__).parameters) == [
        "self", "perturb", "N_importance", "N_samples", "use_viewdirs", "white_bkgd", "raw_noise_std", "ndc", "lindisp", "near", "far"]


# ------------------------------------------------------------------------------------------------ the mirror's own promises
BOXES = [((-1.5, -0.25, -3.0), (1.0, 0.75, 2.0), (5, 7, 33)), ((-1, -1, -1), (1, 1, 1), (1, 1, 1)),
         ((-1.0, 2.0, -6.0), (1.0, 2.5, -2.0), (1024, 1, 1)), ((-1, -1, -1), (1, 1, 1), (1024, 1, 2))]


@pytest.mark.parametrize("lo,hi,n", BOXES)
def test_mirror_samples_look_up_to_their_own_cells(lo, hi, n):
    cells = n[0] * n[1] * n[2]
    for seed in (0, 7, 0xfffffff0):
        pts = M.sample_points(lo, hi, n, 0, cells, 5, seed)
        assert pts.dtype == np.float32 and pts.shape == (cells * 5, 3)
        assert np.array_equal(M.lookup(pts, lo, hi, n), np.repeat(np.arange(cells, dtype=np.int32), 5))
    centre = M.sample_points(lo, hi, n, 0, cells, 1, 3)
    assert np.array_equal(centre, M.sample_points(lo, hi, n, 0, cells, 5, 9)[::5])      # sample 0 does not depend on K or the seed
    sub = M.sample_points(lo, hi, n, cells // 2, cells, 5, 7)
    assert np.array_equal(sub, M.sample_points(lo, hi, n, 0, cells, 5, 7)[5 * (cells // 2):])      # keyed by the global cell index


def test_mirror_mix_is_the_headers_and_words_are_bit_c_of_word_c():
    # mix() by hand in Python integers
    def mix(x):
        x ^= x >> 16; x = x * 0x7feb352d & 0xffffffff; x ^= x >> 15; x = x * 0x846ca68b & 0xffffffff; x ^= x >> 16
        return x
    xs = [0, 1, 0x9e3779b9, 0xffffffff, 123456789]
    with np.errstate(over="ignore"):
        assert [int(v) for v in M.mix(np.array(xs, np.uint32))] == [mix(x) for x in xs]
    rng = np.random.default_rng(0)
    mask = rng.random((5, 7, 33)) < 0.5
    w = M.words(mask).view(np.uint32)
    assert w.shape == (37,) and int(w[-1]) >> (1155 & 31) == 0
    flat = mask.reshape(-1)
    assert all(bool((int(w[c >> 5]) >> (c & 31)) & 1) == bool(flat[c]) for c in range(1155))


@pytest.mark.parametrize("iterations", [1, 2])
def test_mirror_dilation_is_max_pool3d(iterations):
    rng = np.random.default_rng(1)
    mask = rng.random((5, 7, 33)) < 0.03
    ref = torch.from_numpy(mask)[None, None].float()
    for _ in range(iterations):
        ref = torch.nn.functional.max_pool3d(ref, kernel_size=3, stride=1, padding=1)
    assert np.array_equal(M.dilate(mask, iterations), ref[0, 0].numpy() > 0)


def test_mirror_lookup_edges():
    lo, hi, n = (-1.5, -0.25, -3.0), (1.0, 0.75, 2.0), (5, 7, 33)
    pts, expect = edge_points(lo, hi, n)
    assert np.array_equal(M.lookup(pts, lo, hi, n) >= 0, expect)


def edge_points(lo, hi, n):
    """Points on the box's faces, at hi, one ulp either side of lo and hi, outside, +-inf and NaN, with whether the definition
    puts them inside -- decided here from the definition's own arithmetic on the x axis alone (y, z at the box centre)."""
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    mid = ((lo32 + hi32) / 2).astype(np.float32)
    xs = [lo32[0], np.nextafter(lo32[0], np.float32(-np.inf)), np.nextafter(lo32[0], np.float32(np.inf)),
          hi32[0], np.nextafter(hi32[0], np.float32(-np.inf)), np.nextafter(hi32[0], np.float32(np.inf)),
          np.float32(-100), np.float32(100), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan), mid[0]]
    pts = np.array([[x, mid[1], mid[2]] for x in xs], np.float32)
    scale = np.float32(np.float64(n[0]) / (np.float64(hi32[0]) - np.float64(lo32[0])))
    with np.errstate(invalid="ignore"):
        t = np.array([np.float32(np.float32(x - lo32[0]) * scale) for x in xs], np.float32)
        expect = (t >= 0) & (t < np.float32(n[0]))
    assert list(expect[[0, 1, 6, 7, 8, 9, 10, 11]]) == [True, False, False, False, False, False, False, True]      # what nobody disputes
    return pts, expect


# ------------------------------------------------------------------------------------------------ the exact culling test's inputs
# A cell is dead only if EVERY sample in it has sigma <= 0, and the sharpened random field of seed 19 changes sign well inside a
# cell of a 64^3 grid (its sigma is <= 0 at half of all points, at neighbouring samples independently), so the share of culled
# samples falls quickly with the number of samples per cell: on 300 adjacent pixels with 64 + 128 samples the oracle culls 9 %.
# The inputs therefore keep cells at about one sample: rays spread over the whole image (every 533rd pixel) and 32 + 8 samples
# across the 64 cells of the rays' depth range.  The oracle then culls a third of the samples (asserted below).
REAL_CFG = dict(N_samples=32, N_importance=8, near=4.0, far=8.0)


def real_cull_inputs():
    """The rays of the exact culling test: 300 rays of the lego pose, every 533rd pixel of the 400 x 400 image, as the [300, 11]
    batch the renderer takes."""
    K = synth.lego_intrinsics(400, 400)
    ro, rd = synth.rays_np(400, 400, K, synth.LEGO_C2W, np.arange(0, 160000, 533)[:300])
    return synth.ray_batch_np(ro, rd, REAL_CFG["near"], REAL_CFG["far"], True)


def dead_cells(samples, sigma, lo, hi, n):
    """bool [n]: live unless the cell holds at least one sample and every sample in it has sigma <= 0."""
    cell = M.lookup(samples, lo, hi, n)
    assert (cell >= 0).all()
    cells = n[0] * n[1] * n[2]
    held = np.bincount(cell, minlength=cells) > 0
    positive = np.bincount(cell, weights=(sigma > 0).astype(np.float64), minlength=cells) > 0
    return ~(held & ~positive).reshape(n)


def extent(pts):
    """A box around the points with a margin of 1/64 of the extent, as float32."""
    lo, hi = pts.min(0).astype(np.float64), pts.max(0).astype(np.float64)
    pad = (hi - lo) / 64
    return (lo - pad).astype(np.float32), (hi + pad).astype(np.float32)


def test_exact_culling_inputs_cull_a_quarter_on_the_oracle():
    """The CPU oracle's render of the exact culling test's inputs (seeds 1 / 19, x3, REAL_CFG, perturb 0): marking dead
    every cell of a 64^3 grid over the rays' extent whose samples all have sigma <= 0 culls at least a quarter of the samples
    of both passes -- the condition the GPU test relies on, checked where it does not depend on the code under test."""
    import test_gpu_parity as P
    batch = torch.from_numpy(real_cull_inputs())
    cfg = dict(P.BASE, **REAL_CFG)
    coarse, fine = P.cpu_model(1, 3.0, **P.VD), P.cpu_model(19, 3.0, **P.VD)
    two = O.render_rays(O.RenderCfg(**cfg), batch, coarse, fine, retraw=True, retweights=True)
    one = O.render_rays(O.RenderCfg(**dict(cfg, N_importance=0)), batch, coarse, None, retraw=True, retweights=True)
    rays = batch.numpy()
    pc, pf = M.ray_points(rays, one["z_vals"].numpy()).reshape(-1, 3), M.ray_points(rays, two["z_vals"].numpy()).reshape(-1, 3)
    sc, sf = one["raw"][..., 3].numpy().reshape(-1), two["raw"][..., 3].numpy().reshape(-1)
    pts, sigma = np.concatenate([pc, pf]), np.concatenate([sc, sf])
    lo, hi = extent(pts)
    mask = dead_cells(pts, sigma, lo, hi, (64, 64, 64))
    on = M.live(M.lookup(pts, lo, hi, (64, 64, 64)), mask, True)
    culled = 1.0 - on.mean()
    print("oracle: %.1f %% of %d samples culled (coarse %.1f %%, fine %.1f %%); %.1f %% of the cells dead"
          % (100 * culled, on.size, 100 * (1 - on[:pc.shape[0]].mean()), 100 * (1 - on[pc.shape[0]:].mean()), 100 * (1 - mask.mean())))
    assert culled >= 0.25
    assert not (sigma[~on] > 0).any()
