"""The occupancy grid on the device (csrc/occupancy.hip, nerf_shared_amd/occupancy.py, Renderer.occupancy).

Every kernel's result is defined exactly (include/nerf_amd.h, "Occupancy grid"), so everything here is compared for equality:
  * the lookup, the jittered sample points, the dilation and the per-view compaction against tests/occupancy_mirror.py;
  * fill_from_density against model.get_density at the grid's own sample points;
  * a render with an all-live grid against the render without a grid, bit for bit, in every mode the dense path has;
  * a render that really culls against the un-culled render, bit for bit: a sample whose raw sigma is <= 0 has alpha 0, so
    replacing its row by zeros changes no bit of any map; the grid is built from the un-culled render's own sigma so that it
    removes only such samples -- and at least a quarter of all samples (the CPU oracle's figure: tests/test_occupancy_host.py).
Shapes are the smallest that still take every path: 1155 cells (not a multiple of 32, cells straddling words), point counts
around one block of the compaction and past one scan thread's single block, chunks that split a batch unevenly.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")

import occupancy_mirror as M  # noqa: E402
import test_gpu_parity as P  # noqa: E402
import test_occupancy_host as H  # noqa: E402
from nerf_shared_amd import _lib, occupancy, synth  # noqa: E402

gpu = pytest.mark.gpu
lib = _lib.lib
LO, HI, RES = (-1.5, -0.25, -3.0), (1.0, 0.75, 2.0), (5, 7, 33)        # non-cubic, negative lo, 1155 cells
VD156 = dict(P.VD, multires=15, multires_views=6)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


def grid_of(dev, lo, hi, res, mask=None, outside="live"):
    g = occupancy.OccupancyGrid([lo, hi], tuple(res), outside=outside, device=dev)
    if mask is not None:
        g.set_mask(torch.from_numpy(np.ascontiguousarray(mask)).to(dev))
    return g


def random_mask(res, p, seed):
    return np.random.default_rng(seed).random(res) < p


# ================================================================================================ lookup
def lookup_points():
    """Random points in and around the box; every face of every cell on every axis and one ulp either side of it (the other
    axes at random interior positions); the edge cases of H.edge_points; +-inf and NaN on each axis."""
    rng = np.random.default_rng(3)
    lo, hi = np.asarray(LO, np.float32), np.asarray(HI, np.float32)
    ext = hi - lo
    pts = [(lo - 0.1 * ext + rng.random((20000, 3)) * 1.2 * ext).astype(np.float32), H.edge_points(LO, HI, RES)[0]]
    for a in range(3):
        width = np.float32((np.float64(hi[a]) - np.float64(lo[a])) / RES[a])
        faces = (lo[a] + np.arange(RES[a] + 1, dtype=np.float32) * width).astype(np.float32)
        faces[-1] = hi[a]
        x = np.concatenate([faces, np.nextafter(faces, np.float32(-np.inf)), np.nextafter(faces, np.float32(np.inf)),
                            np.array([np.inf, -np.inf, np.nan], np.float32)])
        p = (lo + (0.05 + 0.9 * rng.random((x.size, 3))) * ext).astype(np.float32)
        p[:, a] = x
        pts.append(p)
    return np.concatenate(pts)


@gpu
@pytest.mark.parametrize("outside", ["live", "empty"])
def test_lookup_equals_the_mirror(dev, outside):
    mask = random_mask(RES, 0.5, 11)
    g = grid_of(dev, LO, HI, RES, mask, outside)
    assert np.array_equal(g.words.cpu().numpy(), M.words(mask)) and np.array_equal(g.mask().cpu().numpy(), mask)
    pts = lookup_points()
    cell = M.lookup(pts, LO, HI, RES)
    assert (cell >= 0).sum() > 10000 and (cell < 0).sum() > 5000 and len(np.unique(cell)) == 1156       # the cases are what they claim
    t = torch.from_numpy(pts).to(dev)
    assert np.array_equal(g.cell_index(t).cpu().numpy(), cell)
    assert np.array_equal(g.query(t).cpu().numpy(), M.live(cell, mask, outside == "live"))
    assert g.query(t[:20].reshape(10, 2, 3)).shape == (10, 2) and g.cell_index(t[:20].reshape(10, 2, 3)).shape == (10, 2)
    assert abs(g.occupied_fraction() - mask.mean()) < 1e-12
    fresh = occupancy.OccupancyGrid([LO, HI], RES, device=dev)                                     # a new grid is all live
    assert fresh.occupied_fraction() == 1.0 and int(fresh.words[-1].item()) == (1 << (1155 & 31)) - 1


# ================================================================================================ jitter
@gpu
@pytest.mark.parametrize("lo,hi,res", H.BOXES)
def test_samples_look_up_to_their_own_cells_and_equal_the_mirror(dev, lo, hi, res):
    g = grid_of(dev, lo, hi, res)
    cells = g.n_cells
    own = torch.arange(cells, dtype=torch.int32, device=dev).repeat_interleave(5)
    for seed in (0, 7, 0xfffffff0):
        pts = g.sample_points(0, cells, 5, seed)
        assert torch.equal(g.cell_index(pts), own), "a sample left its cell"
        assert np.array_equal(pts.cpu().numpy(), M.sample_points(lo, hi, res, 0, cells, 5, seed))
    c0 = min(32, cells - 1)
    assert np.array_equal(g.sample_points(c0, cells, 3, 5).cpu().numpy(), M.sample_points(lo, hi, res, c0, cells, 3, 5))
    assert g.sample_points(cells, cells, 4, 0).shape == (0, 3)


# ================================================================================================ fill and dilation
@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32_split"])
@pytest.mark.parametrize("n_models", [1, 2])
def test_fill_equals_get_density_at_the_sample_points(dev, precision, n_models, monkeypatch):
    """dilate=0: mask == any_j(get_density(sample_points) > threshold), ORed over the models.  The fill runs in chunks of 256
    cells here (five chunks, the last one ragged and ending inside a word), the expectation in one piece.  The models are the
    render tests' pair: seed 1 is positive in a seventh of the cells, seed 19 in most, and the pair is given with seed 1 LAST, so a
    fill that kept only the last model's bits would lose most of the grid."""
    monkeypatch.setattr(occupancy, "FILL_CHUNK_POINTS", 1024)
    models = [P.gpu_model(dev, 19, 3.0, precision, **P.VD), P.gpu_model(dev, 1, 3.0, precision, **P.VD)][-n_models:]
    for threshold, seed in ((0.0, 0), (0.75, 5)):
        g = grid_of(dev, LO, HI, RES, random_mask(RES, 0.5, 2))            # what was there before must not survive
        assert g.fill_from_density(models if n_models > 1 else models[0], threshold=threshold, samples_per_cell=4, dilate=0,
                                   seed=seed) is g
        pts = g.sample_points(0, g.n_cells, 4, seed)
        with torch.no_grad():
            expect = torch.zeros(g.n_cells, dtype=torch.bool, device=dev)
            for m in models:
                expect |= (m.get_density(pts).reshape(-1, 4) > threshold).any(1)
        assert 0 < int(expect.sum().item()) < g.n_cells                    # both kinds of cell
        if n_models > 1:
            with torch.no_grad():
                last = (models[-1].get_density(pts).reshape(-1, 4) > threshold).any(1)
            assert int((expect & ~last).sum().item()) > 100                # ... and the first model matters
        assert torch.equal(g.mask().reshape(-1), expect)
        assert int(g.words[-1].item()) >> (1155 & 31) == 0                 # the unused bits stay 0


@gpu
def test_mark_accumulates_and_respects_its_cell_range(dev):
    """nerf_amd_occupancy_mark on its own: cells [32, 100) of 160, K = 3, NaN and the threshold itself compare false; without
    accumulate the touched words' other bits become 0, with accumulate every old bit stays; untouched words are untouched."""
    rng = np.random.default_rng(4)
    sigma = rng.standard_normal((68, 3)).astype(np.float32)
    sigma[5] = [np.nan, -1, -2]
    sigma[6] = [0.25, 0.25, -1]                                             # == threshold: not above it
    on = np.zeros(160, bool)
    with np.errstate(invalid="ignore"):
        on[32:100] = (sigma > np.float32(0.25)).any(1)
    old = random_mask((160,), 0.5, 9)
    s = torch.from_numpy(sigma).to(dev)
    for accumulate in (0, 1):
        w = torch.from_numpy(M.words(old)).to(dev)
        _lib.check(lib.nerf_amd_occupancy_mark(s.data_ptr(), 32, 100, 3, 0.25, accumulate, w.data_ptr(), None), "mark")
        expect = old.copy()
        expect[32:128] = (on[32:128] | old[32:128]) if accumulate else on[32:128]
        torch.cuda.synchronize()
        assert np.array_equal(w.cpu().numpy(), M.words(expect)), accumulate


@gpu
@pytest.mark.parametrize("res", [RES, (1, 1, 1), (3, 40, 2)])
def test_dilation_is_max_pool3d(dev, res):
    mask = random_mask(res, 0.03 if res != (1, 1, 1) else 1.0, 6)
    ref = torch.from_numpy(mask)[None, None].float()
    for iterations in (0, 1, 2):
        g = grid_of(dev, (0, 0, 0), (1, 1, 1), res, mask)
        g.dilate(iterations)
        got = g.mask().cpu()
        assert torch.equal(got, ref[0, 0] > 0), iterations
        assert np.array_equal(got.numpy(), M.dilate(mask, iterations))
        assert np.array_equal(g.words.cpu().numpy(), M.words(got.numpy()))                 # unused bits 0
        ref = torch.nn.functional.max_pool3d(ref, kernel_size=3, stride=1, padding=1)


# ================================================================================================ compaction
CB_LO, CB_HI, CB_RES = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0), (8, 8, 8)


def checkerboard():
    i = np.indices(CB_RES).sum(0)
    return (i & 1) == 0


def cull_rays(R, ray_ch, seed):
    """Rays that start around the box and cross it, with depths that put samples inside and outside."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.4, 1.4, (R, 3))
    d = rng.standard_normal((R, 3))
    rays = np.concatenate([o, d, np.zeros((R, 1)), np.ones((R, 1)), d / np.linalg.norm(d, axis=1, keepdims=True)], 1).astype(np.float32)
    return np.ascontiguousarray(rays[:, :ray_ch])


def run_cull(dev, g, rays, z):
    R, S = z.shape
    n = R * S
    r, zz = torch.from_numpy(rays).to(dev), torch.from_numpy(z).to(dev)
    rank = torch.full((n,), -7, dtype=torch.int32, device=dev)
    counts = torch.empty((n + 255) // 256, dtype=torch.int32, device=dev)
    pts = torch.full((n, 3), 9.0, device=dev)
    vd = torch.full((n, 3), 9.0, device=dev) if rays.shape[1] == 11 else None
    count = torch.full((1,), -1, dtype=torch.int64, device=dev)
    c = g._c()
    _lib.check(lib.nerf_amd_occupancy_cull(ctypes.byref(c), r.data_ptr(), rays.shape[1], zz.data_ptr(), R, S, counts.data_ptr(),
                                           rank.data_ptr(), pts.data_ptr(), _lib.ptr(vd), count.data_ptr(), None), "cull")
    torch.cuda.synchronize()
    return rank, int(count.item()), pts, vd


@gpu
@pytest.mark.parametrize("R,S,ray_ch", [(1, 1, 11), (5, 51, 8), (4, 64, 11), (1, 257, 11), (1025, 64, 11)])
@pytest.mark.parametrize("outside", ["live", "empty"])
def test_compaction_equals_the_mirror(dev, R, S, ray_ch, outside):
    """rank, count, pts_live, vd_live on a checkerboard; R S = 1, 255, 256, 257 and 65 600 (257 blocks: past the 256 threads of
    the scan's block, so its threads own runs of two).  Then expand: live rows from their rank, +0.0 elsewhere."""
    mask = checkerboard()
    g = grid_of(dev, CB_LO, CB_HI, CB_RES, mask, outside)
    rays = cull_rays(R, ray_ch, R + S)
    z = np.sort(np.random.default_rng(S).uniform(-1.5, 1.5, (R, S)).astype(np.float32), axis=1)
    rank, count, pts, vd = run_cull(dev, g, rays, z)
    m_rank, m_count, m_pts, m_vd = M.cull(rays, z, mask, CB_LO, CB_HI, outside == "live")
    if R * S > 1:
        assert 0 < m_count < R * S
    assert count == m_count
    assert np.array_equal(rank.cpu().numpy(), m_rank)
    assert np.array_equal(pts[:count].cpu().numpy(), m_pts)
    assert torch.all(pts[count:] == 9.0)                                                   # nothing written past the list
    if ray_ch == 11:
        assert np.array_equal(vd[:count].cpu().numpy(), m_vd) and torch.all(vd[count:] == 9.0)
    for ch in (4, 5):
        live = torch.from_numpy(np.random.default_rng(ch).standard_normal((max(count, 1), ch)).astype(np.float32)).to(dev)
        raw = torch.full((R * S, ch), 7.0, device=dev)
        _lib.check(lib.nerf_amd_occupancy_expand(live.data_ptr(), rank.data_ptr(), R * S, ch, raw.data_ptr(), None), "expand")
        expect = np.where(m_rank[:, None] >= 0, live.cpu().numpy()[np.maximum(m_rank, 0)], np.float32(0.0))
        got = raw.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), expect.astype(np.float32).view(np.uint32))      # bits: the zeros are +0.0


@gpu
@pytest.mark.parametrize("live", [False, True])
def test_compaction_all_dead_and_all_live(dev, live):
    mask = np.full(CB_RES, live)
    g = grid_of(dev, CB_LO, CB_HI, CB_RES, mask, "live" if live else "empty")
    rays = cull_rays(9, 11, 1)
    z = np.random.default_rng(2).uniform(-1.5, 1.5, (9, 64)).astype(np.float32)
    rank, count, pts, vd = run_cull(dev, g, rays, z)
    if live:
        assert count == 576 and torch.equal(rank, torch.arange(576, dtype=torch.int32, device=dev))
        assert np.array_equal(pts.cpu().numpy(), M.ray_points(rays, z).reshape(-1, 3))
        assert np.array_equal(vd.cpu().numpy(), np.repeat(rays[:, 8:11], 64, axis=0))
    else:
        assert count == 0 and torch.all(rank == -1) and torch.all(pts == 9.0) and torch.all(vd == 9.0)


@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32_split", "fp32"])
def test_field_points_is_the_render_paths_field(dev, precision):
    """nerf_amd_field_points at explicit points with one view direction per point equals the raw the dense render returns for
    the same points (rays + z_vals mode, the render path's weight stream); n = 0 is accepted and launches nothing."""
    _, render_utils, _ = P.amd()
    c = P.gpu_model(dev, 1, 3.0, precision, **P.VD)
    batch = torch.from_numpy(H.real_cull_inputs()[:37]).to(dev)
    r = render_utils.Renderer(**dict(P.BASE, N_importance=0))
    with torch.no_grad():
        out = r.render_rays(batch, c, None, retraw=True, retweights=True)
    pts = torch.from_numpy(M.ray_points(batch.cpu().numpy(), out["z_vals"].cpu().numpy()).reshape(-1, 3)).to(dev)
    vd = batch[:, 8:11].repeat_interleave(64, dim=0).contiguous()
    raw = torch.empty(pts.shape[0], 4, device=dev)
    copies = _lib.COPY_OF[c._precision_code()] | (_lib.COPY_BF16_FOLD if precision == "bf16" else 0)
    h = c._model_handle(dev, copies)
    _lib.check(lib.nerf_amd_field_points(h, pts.data_ptr(), vd.data_ptr(), pts.shape[0], raw.data_ptr(), c._precision_code(), None), "field_points")
    torch.cuda.synchronize()
    assert torch.equal(raw.reshape(37, 64, 4), out["raw"])
    assert lib.nerf_amd_field_points(h, None, None, 0, None, c._precision_code(), None) == 0


# ================================================================================================ all-live grid == no grid
def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape, k
        assert torch.equal(torch.isnan(a[k]), torch.isnan(b[k])), k
        assert torch.equal(torch.nan_to_num(a[k]), torch.nan_to_num(b[k])), k


def lego_batch(dev, n=300, use_viewdirs=True, ndc=False, near=2.0, far=6.0):
    _, _, utils = P.amd()
    K = synth.lego_intrinsics(400, 400)
    return utils.make_ray_batch(400, 400, K, synth.LEGO_C2W, near, far, use_viewdirs, ndc, device=dev, pix0=70000, n=n)


ALL_LIVE_CASES = {
    "bf16": dict(),
    "fp32_split": dict(precision="fp32_split"),
    "fp32": dict(precision="fp32"),
    "bf16_15_6": dict(arch=VD156),
    "no_view_branch": dict(arch=P.NOVD),
    "perturbed": dict(cfg=dict(perturb=1.0)),
    "coarse_only": dict(cfg=dict(N_importance=0)),
    "fine_is_coarse": dict(fine=False),
    "lindisp": dict(cfg=dict(lindisp=True)),
    "ndc_64_64": dict(cfg=dict(ndc=True, near=0.0, far=1.0, N_importance=64), ndc=True),
}


@gpu
@pytest.mark.parametrize("name", list(ALL_LIVE_CASES))
def test_all_live_grid_equals_no_grid(dev, name):
    """300 rays, chunk 128 (three uneven chunks), through render_rays (retraw, retweights) and render_batch (retraw): with a grid
    whose every cell is live and whose outside is live, every returned key equals the dense path's, NaN patterns included.
    The perturbed case renders with pytest=True (render_rays) and from a reseeded generator (render_batch)."""
    case = ALL_LIVE_CASES[name]
    _, render_utils, _ = P.amd()
    arch, precision = case.get("arch", P.VD), case.get("precision", "bf16")
    cfg = dict(P.BASE, use_viewdirs=arch["use_viewdirs"], **case.get("cfg", {}))
    c = P.gpu_model(dev, 1, 3.0, precision, **arch)
    f = P.gpu_model(dev, 19, 3.0, precision, **arch) if case.get("fine", True) else None
    batch = lego_batch(dev, 300, arch["use_viewdirs"], case.get("ndc", False), cfg["near"], cfg["far"])
    r = render_utils.Renderer(**cfg)
    grid = grid_of(dev, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (5, 7, 33))            # many points inside, many outside: all live
    perturbed = cfg["perturb"] > 0

    def both():
        with torch.no_grad():
            torch.manual_seed(3)
            a = r.render_rays(batch, c, f, retraw=True, retweights=True, pytest=perturbed)
            torch.manual_seed(4)
            b = r.render_batch(c, f, batch, chunk=128, retraw=True)
        torch.cuda.synchronize()
        return a, b

    dense = both()
    r.occupancy = grid
    culled = both()
    same(culled[0], dense[0])
    same(culled[1], dense[1])
    fine_points = 300 * (64 + cfg["N_importance"]) if cfg["N_importance"] else 0          # (of render_batch, the last call)
    assert r.last_cull == {"coarse_live": 300 * 64, "coarse_total": 300 * 64, "fine_live": fine_points, "fine_total": fine_points}


# ================================================================================================ real culling, exact oracle
MAPS = ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "z_std", "z_vals", "weights")


@gpu
def test_real_culling_is_exact_where_sigma_is_not_positive(dev):
    """bf16 models of seeds 1 / 19, x3 (tests/test_gpu_fold.py), the 300 rays and sample counts of H.REAL_CFG (chosen there so
    that cells hold about one sample), perturb 0, coarse-only and two-pass.
    1. render un-culled; 2. a cell of a 64^3 grid over the samples' extent is dead iff it holds a sample (coarse or fine) and
    every sample in it has raw sigma <= 0; 3. the culled renders equal the un-culled ones bit for bit in every map, in z_vals and
    weights, and in raw at live samples, with all-zero rows elsewhere; 4. last_cull equals the mirror's counts; 5. at least a
    quarter of all samples are culled (the CPU oracle culls a third: tests/test_occupancy_host.py)."""
    _, render_utils, _ = P.amd()
    c, f = P.gpu_model(dev, 1, 3.0, "bf16", **P.VD), P.gpu_model(dev, 19, 3.0, "bf16", **P.VD)
    rays = H.real_cull_inputs()
    batch = torch.from_numpy(rays).to(dev)
    r1, r2 = render_utils.Renderer(**dict(P.BASE, **dict(H.REAL_CFG, N_importance=0))), render_utils.Renderer(**dict(P.BASE, **H.REAL_CFG))

    def render(r):
        with torch.no_grad():
            out = r.render_rays(batch, c, f, retraw=True, retweights=True)
        torch.cuda.synchronize()
        return {k: v.cpu() for k, v in out.items()}

    one, two = render(r1), render(r2)
    pc = M.ray_points(rays, one["z_vals"].numpy()).reshape(-1, 3)
    pf = M.ray_points(rays, two["z_vals"].numpy()).reshape(-1, 3)
    sigma = np.concatenate([one["raw"][..., 3].numpy().reshape(-1), two["raw"][..., 3].numpy().reshape(-1)])
    pts = np.concatenate([pc, pf])
    assert not np.isnan(sigma).any()
    lo, hi = H.extent(pts)
    mask = H.dead_cells(pts, sigma, lo, hi, (64, 64, 64))
    on_c = M.live(M.lookup(pc, lo, hi, (64, 64, 64)), mask, True)
    on_f = M.live(M.lookup(pf, lo, hi, (64, 64, 64)), mask, True)
    culled = 1.0 - (on_c.sum() + on_f.sum()) / (on_c.size + on_f.size)
    print("culled %.1f %% of %d samples (coarse %.1f %%, fine %.1f %%)" % (100 * culled, on_c.size + on_f.size, 100 * (1 - on_c.mean()), 100 * (1 - on_f.mean())))
    assert culled >= 0.25
    grid = grid_of(dev, lo, hi, (64, 64, 64), mask, "live")
    r1.occupancy = r2.occupancy = grid
    got1, got2 = render(r1), render(r2)
    assert r1.last_cull == {"coarse_live": int(on_c.sum()), "coarse_total": on_c.size, "fine_live": 0, "fine_total": 0}
    assert r2.last_cull == {"coarse_live": int(on_c.sum()), "coarse_total": on_c.size, "fine_live": int(on_f.sum()), "fine_total": on_f.size}
    for got, ref, on in ((got1, one, on_c), (got2, two, on_f)):
        for k in MAPS:
            if k in ref:
                assert torch.equal(torch.isnan(got[k]), torch.isnan(ref[k])) and torch.equal(torch.nan_to_num(got[k]), torch.nan_to_num(ref[k])), k
        on_t = torch.from_numpy(on).reshape(ref["raw"].shape[:2])
        assert torch.equal(got["raw"][on_t], ref["raw"][on_t])
        assert torch.all(got["raw"][~on_t].view(torch.int32) == 0)                       # +0.0 in every channel
    assert "rgb0" in got2 and "rgb0" not in got1
    # render_batch in uneven chunks culls the same samples
    with torch.no_grad():
        b = r2.render_batch(c, f, batch, chunk=128, retraw=True)
    torch.cuda.synchronize()
    assert r2.last_cull == {"coarse_live": int(on_c.sum()), "coarse_total": on_c.size, "fine_live": int(on_f.sum()), "fine_total": on_f.size}
    for k in ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "z_std"):
        assert torch.equal(torch.nan_to_num(b[k].cpu()), torch.nan_to_num(two[k])), k


@gpu
@pytest.mark.parametrize("two_pass", [False, True])
def test_all_dead_grid_renders_the_background(dev, two_pass):
    """No live point: no field kernel runs, raw is all zero, acc == 0 and the colour is the white background."""
    _, render_utils, _ = P.amd()
    c, f = P.gpu_model(dev, 1, 3.0, "bf16", **P.VD), P.gpu_model(dev, 19, 3.0, "bf16", **P.VD)
    batch = lego_batch(dev, 130)
    r = render_utils.Renderer(**dict(P.BASE, N_importance=128 if two_pass else 0))
    r.occupancy = grid_of(dev, (-1, -1, -1), (1, 1, 1), (4, 4, 4), np.zeros((4, 4, 4), bool), "empty")
    launches = (ctypes.c_int64 * 3)()
    ms, points = (ctypes.c_double * 3)(), (ctypes.c_double * 3)()
    lib.nerf_amd_profile_enable(1)
    try:
        lib.nerf_amd_profile_collect(launches, ms, points)                      # forget whatever was recorded before
        with torch.no_grad():
            out = r.render_rays(batch, c, f, retraw=True, retweights=True)
        torch.cuda.synchronize()
        _lib.check(lib.nerf_amd_profile_collect(launches, ms, points), "profile_collect")
    finally:
        lib.nerf_amd_profile_enable(0)
    assert list(launches) == [0, 0, 0]
    S = 192 if two_pass else 64
    assert r.last_cull == {"coarse_live": 0, "coarse_total": 130 * 64, "fine_live": 0, "fine_total": 130 * 192 if two_pass else 0}
    assert out["raw"].shape == (130, S, 4) and torch.all(out["raw"].view(torch.int32) == 0)
    assert torch.all(out["acc_map"] == 0) and torch.all(out["rgb_map"] == 1) and torch.all(out["weights"] == 0)
    if two_pass:
        assert torch.all(out["acc0"] == 0) and torch.all(out["rgb0"] == 1)


# ================================================================================================ refusals
@gpu
def test_grid_refuses_gradients_and_noise_and_leaves_nothing_behind(dev):
    _, render_utils, _ = P.amd()
    c, f = P.gpu_model(dev, 1, 3.0, "bf16", **P.VD), P.gpu_model(dev, 19, 3.0, "bf16", **P.VD)
    batch = lego_batch(dev, 64)
    r = render_utils.Renderer(**P.BASE)
    r.occupancy = grid_of(dev, (-1, -1, -1), (1, 1, 1), (4, 4, 4), random_mask((4, 4, 4), 0.5, 1), "empty")
    c.requires_grad_(True)
    for call in (lambda: r.render_rays(batch, c, f), lambda: r.render_batch(c, f, batch, chunk=32),
                 lambda: r.render(8, 8, synth.lego_intrinsics(8, 8), c, f, c2w=torch.from_numpy(synth.LEGO_C2W))):
        with pytest.raises(_lib.NerfAmdError, match="occupancy = None"):
            call()
    with torch.no_grad():
        r.render_rays(batch, c, f)                                            # the same call without a gradient request renders
    c.requires_grad_(False)
    with pytest.raises(_lib.NerfAmdError, match="occupancy = None"):
        r.render_rays(batch.clone().requires_grad_(True), c, f)               # gradients for the rays (pose estimation)
    noisy = render_utils.Renderer(**dict(P.BASE, raw_noise_std=1.0))
    noisy.occupancy = r.occupancy
    for call in (lambda: noisy.render_rays(batch, c, f), lambda: noisy.render_batch(c, f, batch)):
        with pytest.raises(_lib.NerfAmdError, match="raw_noise_std"):
            call()
    with pytest.raises(_lib.NerfAmdError, match="no CPU path"):
        r.render_rays(batch.cpu(), c, f)
    # switched off again, the renderer is the dense one
    culled = r.render_rays(batch, c, f, retraw=True, retweights=True)
    r.occupancy = None
    back = r.render_rays(batch, c, f, retraw=True, retweights=True)
    fresh = render_utils.Renderer(**P.BASE).render_rays(batch, c, f, retraw=True, retweights=True)
    torch.cuda.synchronize()
    same(back, fresh)
    assert not torch.equal(culled["raw"], fresh["raw"])                       # (the grid had been doing something)
