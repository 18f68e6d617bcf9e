"""CPU tests of the occupancy grid's training surface: the three new C entry points are bound with the header's signatures and
refuse bad grids and arguments before any launch, occupancy.TrainCull refuses bad fractions and sizes its lists as documented,
Renderer.train_occupancy defaults to None -- and the mirror (tests/train_cull_mirror.py) keeps its own promises: the capped cull
is the uncapped one when the capacity covers the live points, the ray-gradient reduction follows the header's order term by
term, and the inputs of tests/test_gpu_train_cull.py keep at least a quarter AND cull at least a quarter of their samples in
both passes on the CPU oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import occupancy_mirror as M  # noqa: E402
import test_gpu_parity as P  # noqa: E402
import test_occupancy_host as H  # noqa: E402
import train_cull_mirror as T  # noqa: E402
from nerf_shared_amd import _lib, occupancy, render_utils, synth  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402

lib = _lib.lib
NEW = ("nerf_amd_occupancy_cull_capped", "nerf_amd_occupancy_gather_rows", "nerf_amd_occupancy_ray_grads")


def test_new_symbols_are_bound_with_the_headers_signatures():
    with open(os.path.join(REPO, "include", "nerf_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        m = re.search(r"(int64_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, name
        args = []
        for a in m.group(2).split(","):
            ctype = re.sub(r"\s*\w+\s*$", "", " ".join(a.split()))           # drop the parameter name
            args.append(ctypes.c_void_p if ctype == "int64_t *" else H.C_TYPES[ctype])      # counts: a DEVICE pointer
        fn = getattr(lib, name)
        assert name in _lib.EXPORTS
        assert fn.restype is H.C_TYPES[m.group(1)], name
        assert list(fn.argtypes) == args, (name, fn.argtypes, args)
    assert lib.nerf_amd_abi_version() == _lib.ABI_VERSION == 7          # additive: the version stays


@pytest.mark.parametrize("bad", [dict(n=(0, 4, 4)), dict(n=(4, 1025, 4)), dict(lo=(1, -1, -1)), dict(hi=(float("inf"), 1, 1)),
                                 dict(lo=(float("nan"), -1, -1)), dict(outside=2), dict(words=None)])
def test_bad_grids_are_refused_before_any_launch(bad):
    g = H._grid(**bad)
    assert lib.nerf_amd_occupancy_cull_capped(ctypes.byref(g), 1, 8, 1, 1, 1, 1, 1, 1, 1, 1, None, 1, None) == -1
    assert lib.nerf_amd_last_error()


def test_bad_arguments_are_refused_before_any_launch():
    g = ctypes.byref(H._grid())
    assert lib.nerf_amd_occupancy_cull_capped(None, 1, 8, 1, 1, 1, 1, 1, 1, 1, 1, None, 1, None) == -1
    assert lib.nerf_amd_occupancy_cull_capped(g, 1, 8, 1, 1, 1, 0, 1, 1, 1, 1, None, 1, None) == -1             # capacity < 1
    assert lib.nerf_amd_occupancy_cull_capped(g, 1, 8, 1, 1, 1, 1 << 31, 1, 1, 1, 1, None, 1, None) == -1
    assert lib.nerf_amd_occupancy_cull_capped(g, 1, 9, 1, 1, 1, 1, 1, 1, 1, 1, None, 1, None) == -1             # ray_ch
    assert lib.nerf_amd_occupancy_cull_capped(g, 1, 8, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == -1                # vd_live without view columns
    assert lib.nerf_amd_occupancy_cull_capped(g, 1, 8, 1, -1, 1, 1, 1, 1, 1, 1, None, 1, None) == -1            # R < 0
    assert lib.nerf_amd_occupancy_cull_capped(g, 1, 8, 1, 1, 0, 1, 1, 1, 1, 1, None, 1, None) == -1             # S < 1
    assert lib.nerf_amd_occupancy_cull_capped(g, 1, 8, 1, 1 << 26, 32, 1, 1, 1, 1, 1, None, 1, None) == -1      # R S = 2^31
    assert lib.nerf_amd_occupancy_cull_capped(g, 1, 8, 1, 1, 1, 1, 1, 1, None, 1, None, 1, None) == -1          # no src
    assert lib.nerf_amd_occupancy_cull_capped(g, 1, 8, 1, 1, 1, 1, 1, 1, 1, None, None, 1, None) == -1          # no pts_live
    assert lib.nerf_amd_occupancy_cull_capped(g, 1, 8, 1, 1, 1, 1, 1, 1, 1, 1, None, None, None) == -1          # no counts
    assert lib.nerf_amd_occupancy_cull_capped(g, None, 8, 1, 1, 1, 1, 1, 1, 1, 1, None, 1, None) == -1          # no rays with R > 0
    assert lib.nerf_amd_occupancy_gather_rows(None, None, 5, 4, None, None) == -1
    assert lib.nerf_amd_occupancy_gather_rows(1, 1, -1, 4, 1, None) == -1
    assert lib.nerf_amd_occupancy_gather_rows(1, 1, 5, 0, 1, None) == -1
    assert lib.nerf_amd_occupancy_gather_rows(None, None, 0, 4, None, None) == 0
    assert lib.nerf_amd_occupancy_ray_grads(None, None, None, None, 3, 4, 8, None, None) == -1
    assert lib.nerf_amd_occupancy_ray_grads(1, 1, 1, None, 3, 4, 9, 1, None) == -1                              # ray_ch
    assert lib.nerf_amd_occupancy_ray_grads(1, 1, 1, 1, 3, 4, 8, 1, None) == -1                                 # g_vd without view columns
    assert lib.nerf_amd_occupancy_ray_grads(1, 1, 1, None, -1, 4, 8, 1, None) == -1
    assert lib.nerf_amd_occupancy_ray_grads(1, 1, 1, None, 3, 0, 8, 1, None) == -1
    assert lib.nerf_amd_occupancy_ray_grads(None, None, None, None, 0, 4, 8, None, None) == 0


def test_train_cull_refuses_bad_fractions_and_sizes_its_lists_as_documented():
    g = occupancy.OccupancyGrid([[-1, -1, -1], [1, 1, 1]], 4, device="cuda:0")          # building either touches no device
    for bad in (0, 0.0, -0.1, 1.5, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="coarse_fraction"):
            occupancy.TrainCull(g, coarse_fraction=bad)
        with pytest.raises(ValueError, match="fine_fraction"):
            occupancy.TrainCull(g, fine_fraction=bad)
    with pytest.raises(TypeError):
        occupancy.TrainCull(None)
    c = occupancy.TrainCull(g)
    assert (c.coarse_fraction, c.fine_fraction, c.grid) == (1.0, 1.0, g)
    c = occupancy.TrainCull(g, 0.25, 1e-9)
    for n in (1, 3, 420, 770, 65536):
        assert c.capacity(False, n) == T.capacity(0.25, n) == min(n, max(1, -(-n // 4)))
        assert c.capacity(True, n) == T.capacity(1e-9, n) == 1
        assert occupancy.TrainCull(g).capacity(False, n) == n
    with pytest.raises(ValueError, match="margin"):
        c.calibrate(0.5)
    with pytest.raises(ValueError, match="cells"):
        g.refresh_from_density([], cells=(16, 64))                 # c0 not a multiple of 32 (refused before any device work)
    with pytest.raises(ValueError, match="cells"):
        g.refresh_from_density([], cells=(0, 40))                  # c1 inside a word
    with pytest.raises(ValueError, match="at least one model"):
        g.refresh_from_density([], cells=(0, 32))
    assert [g.slab(i, 2) for i in range(3)] == [(0, 32), (32, 64), (0, 32)]
    big = occupancy.OccupancyGrid([[-1, -1, -1], [1, 1, 1]], (5, 7, 33), device="cuda:0")       # 1155 cells, 37 words
    slabs = [big.slab(i, 4) for i in range(4)]
    assert slabs[0][0] == 0 and slabs[-1][1] == 1155 and all(a[1] == b[0] and b[0] % 32 == 0 for a, b in zip(slabs, slabs[1:]))


def test_renderer_train_occupancy_defaults_to_none():
    assert render_utils.Renderer.train_occupancy is None
    r = render_utils.Renderer(perturb=0.0)
    assert r.train_occupancy is None and "train_occupancy" not in r.__dict__ and "train_occupancy" not in r.state_dict()
    assert r.occupancy is None


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
# 70 rays of the lego pose spread over the image, 6 + 5 samples: 420 and 770 points -- several 256-point blocks of the
# compaction, not a multiple of 64, and a fine pass.  A 4^3 grid over [-1.8, 1.8]^3: most samples are inside (the mask
# decides), the first and last depths of many rays outside (the outside policy decides).
R, NC, NI = 70, 6, 5
CFG = dict(P.BASE, N_samples=NC, N_importance=NI)
LO, HI, RES = (-1.8, -1.8, -1.8), (1.8, 1.8, 1.8), (4, 4, 4)
MASK_SEED = 0
ARCH = {11: P.VD, 8: P.NOVD}


def batch_np(ray_ch):
    K = synth.lego_intrinsics(400, 400)
    ro, rd = synth.rays_np(400, 400, K, synth.LEGO_C2W, np.arange(311, 160000, 2287)[:R])
    b = synth.ray_batch_np(ro, rd, CFG["near"], CFG["far"], True)
    assert b.shape == (R, 11)
    return np.ascontiguousarray(b[:, :ray_ch])


def half_live_mask():
    return np.random.default_rng(MASK_SEED).random(RES) < 0.5


_DEPTHS = {}


def oracle_depths(ray_ch):
    """(z_coarse [R, NC], z_fine [R, NC + NI]) of the CPU oracle's render of the GPU tests' inputs (seeds 1 / 19, x3, perturb 0)."""
    if ray_ch not in _DEPTHS:
        batch = torch.from_numpy(batch_np(ray_ch))
        coarse, fine = P.cpu_model(1, 3.0, **ARCH[ray_ch]), P.cpu_model(19, 3.0, **ARCH[ray_ch])
        cfg = dict(CFG, use_viewdirs=ray_ch == 11)
        two = O.render_rays(O.RenderCfg(**cfg), batch, coarse, fine, retweights=True)
        one = O.render_rays(O.RenderCfg(**dict(cfg, N_importance=0)), batch, coarse, None, retweights=True)
        _DEPTHS[ray_ch] = one["z_vals"].numpy().astype(np.float32), two["z_vals"].numpy().astype(np.float32)
    return _DEPTHS[ray_ch]


@pytest.mark.parametrize("ray_ch", [8, 11])
@pytest.mark.parametrize("outside", ["live", "empty"])
def test_gpu_test_inputs_keep_a_quarter_and_cull_a_quarter_on_the_oracle(ray_ch, outside):
    rays, mask = batch_np(ray_ch), half_live_mask()
    assert 0.4 < mask.mean() < 0.6
    for name, z in zip(("coarse", "fine"), oracle_depths(ray_ch)):
        pts = M.ray_points(rays, z).reshape(-1, 3)
        cell = M.lookup(pts, LO, HI, RES)
        on = M.live(cell, mask, outside == "live")
        print("%s ray_ch %d outside %s: %d points, %.1f %% live, %.1f %% outside the box"
              % (name, ray_ch, outside, on.size, 100 * on.mean(), 100 * (cell < 0).mean()))
        assert on.size == R * z.shape[1] and 0.25 <= on.mean() <= 0.75
        assert (cell < 0).sum() >= 20                                  # the outside policy decides something


# ------------------------------------------------------------------------------------------------ the mirror's own promises
@pytest.mark.parametrize("ray_ch", [8, 11])
def test_capped_mirror_is_the_uncapped_mirror_when_the_capacity_covers_the_live_points(ray_ch):
    rays, mask = batch_np(ray_ch), half_live_mask()
    z = oracle_depths(ray_ch)[1]
    rank0, live, pts0, vd0 = M.cull(rays, z, mask, LO, HI, False)
    n = z.size
    for cap in (live, live + 1, n):
        rank, src, pts, vd, counts = T.cull_capped(rays, z, mask, LO, HI, False, cap)
        assert counts == (live, live) and np.array_equal(rank, rank0)
        assert np.array_equal(pts[:live], pts0) and (vd0 is None) == (vd is None) and (vd is None or np.array_equal(vd[:live], vd0))
        assert np.array_equal(src[:live], np.nonzero(rank0 >= 0)[0]) and np.array_equal(rank[src[:live]], np.arange(live))
        assert (src[live:] == -1).all() and (pts[live:] == T.centre(LO, HI)).all() and (vd is None or (vd[live:] == [0, 0, 1]).all())
    cap = live // 3
    rank, src, pts, vd, counts = T.cull_capped(rays, z, mask, LO, HI, False, cap)
    assert counts == (live, cap) and (src >= 0).all()
    assert np.array_equal(rank >= 0, (rank0 >= 0) & (rank0 < cap)) and np.array_equal(rank[rank >= 0], np.arange(cap))
    assert np.array_equal(pts, pts0[:cap])
    x = np.random.default_rng(1).standard_normal((cap, 4)).astype(np.float32)
    assert np.array_equal(T.gather_rows(T.expand(x, rank), src), x)
    assert T.cull_capped(rays[:0], z[:0], mask, LO, HI, False, 3)[4] == (0, 0)


def _ray_grads_by_hand(rank, z, g_pts, g_vd, ray_ch):
    """The header's order in scalar float32 operations: nothing vectorised, nothing shared with the mirror."""
    f = np.float32
    Rn, S = z.shape
    out = np.zeros((Rn, ray_ch), f)
    for r in range(Rn):
        cols = {}
        for c in range(9):
            lane = [f(0.0)] * 64
            for l in range(64):
                for s in range(l, S, 64):
                    row = rank[r * S + s]
                    if row < 0:
                        continue
                    if c < 3:
                        term = g_pts[row, c]
                    elif c < 6:
                        term = f(g_pts[row, c - 3] * z[r, s])
                    else:
                        term = g_vd[row, c - 6] if g_vd is not None else None
                    if term is not None:
                        lane[l] = f(lane[l] + term)
            for m in (32, 16, 8, 4, 2, 1):
                lane = [f(lane[l] + lane[l ^ m]) for l in range(64)]
            cols[c] = lane[0]
        for c in range(6):
            out[r, c] = cols[c]
        if ray_ch == 11:
            for c in range(3):
                out[r, 8 + c] = cols[6 + c]
    return out


@pytest.mark.parametrize("S,ray_ch,with_vd", [(11, 11, True), (130, 11, True), (64, 8, False), (1, 11, False), (200, 11, True)])
def test_ray_gradient_mirror_follows_the_headers_order(S, ray_ch, with_vd):
    rng = np.random.default_rng(S)
    Rn = 5
    kept = rng.random(Rn * S) < 0.6
    kept[:S] = S > 1                                    # one ray whole (a lone sample: culled -> an exact zero row)
    rank = np.where(kept, np.cumsum(kept) - 1, -1).astype(np.int32)
    C = int(kept.sum()) + 3
    z = np.sort(rng.uniform(2, 6, (Rn, S)).astype(np.float32), -1)
    g_pts = (rng.standard_normal((C, 3)) * 10.0 ** rng.integers(-6, 3, (C, 1))).astype(np.float32)     # sums whose order shows
    g_vd = rng.standard_normal((C, 3)).astype(np.float32) if with_vd else None
    got = T.ray_grads(rank, z, g_pts, g_vd, ray_ch)
    ref = _ray_grads_by_hand(rank, z, g_pts, g_vd, ray_ch)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert (got[:, 6:8] == 0).all()
    if S >= 64:          # the order is not a plain left-to-right sum (so the comparison above means something)
        naive = np.zeros((Rn, 3), np.float32)
        for r in range(Rn):
            for s in range(S):
                if rank[r * S + s] >= 0:
                    naive[r] = (naive[r] + g_pts[rank[r * S + s]]).astype(np.float32)
        assert not np.array_equal(naive, got[:, 0:3])
        np.testing.assert_allclose(naive, got[:, 0:3], rtol=1e-3, atol=1e-3)
