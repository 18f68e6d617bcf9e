"""The occupancy grid in training and pose estimation on the device (occupancy.TrainCull, Renderer.train_occupancy; the
kernels nerf_amd_occupancy_cull_capped / _gather_rows / _ray_grads of csrc/occupancy.hip; OccupancyGrid.refresh_from_density).

  1. the three kernels against tests/train_cull_mirror.py, bit for bit;
  2. an all-live grid at fraction 1.0 against the dense training call, bit for bit, in the three precisions, perturbed;
  3. a half-live grid against a restatement built here from public ops and torch indexing (the mirror's padded list ->
     model.forward in train mode -> index_put into zeros -> raw2outputs): outputs and parameter gradients bit for bit; tensors
     that a float atomic or torch's index_add accumulates (the head of a model without view branch, the ray gradients of the
     restatement) under the fp32-reordering gate of test_raw2outputs_backward_matches_autograd;
  4. the semantics against fp32 autograd of the CPU oracle with raw multiplied by the kept mask, precision 'fp32';
  5. overflow at fraction 0.25;  6. refusals and defaults;  7. captured steps, and the grid refreshed between replays.
The shapes are tests/test_train_cull_host.py's: 70 rays, 6 + 5 samples (420 and 770 points), a 4^3 grid with a random half-live
mask, `outside` both ways, rays with and without view columns -- that file shows on the CPU oracle that they keep at least a
quarter and cull at least a quarter of the samples in both passes."""
import ctypes
import os

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")

import occupancy_mirror as M  # noqa: E402
import test_gpu_parity as P  # noqa: E402
import test_train_cull_host as H  # noqa: E402
import train_cull_mirror as T  # noqa: E402
from nerf_shared_amd import _lib, occupancy, synth  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402
from test_gpu_backward import rel_err  # noqa: E402
from test_gpu_occupancy import grid_of  # noqa: E402

gpu = pytest.mark.gpu
lib = _lib.lib
R, NC, NI, LO, HI, RES = H.R, H.NC, H.NI, H.LO, H.HI, H.RES
PRECISIONS = ["bf16", "fp32_split", "fp32"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a ROCm device"
    return torch.device("cuda:0")


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def reordering_gate(got, ref):
    """The gate test_raw2outputs_backward_matches_autograd uses for fp32 sums taken in another order."""
    got, ref = got.detach().cpu().numpy(), ref.detach().cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=2e-5 * float(np.abs(ref).max()), rtol=2e-4)


def models_of(dev, ray_ch, precision, train=True):
    ms = [P.gpu_model(dev, seed, 3.0, precision, **H.ARCH[ray_ch]) for seed in (1, 19)]
    for m in ms:
        m.requires_grad_(train)
    return ms


def renderer(**over):
    from nerf_shared_amd import render_utils
    return render_utils.Renderer(**dict(H.CFG, **over))


# ================================================================================================ 1. the kernels
def run_cull(dev, grid, rays, z, cap):
    """nerf_amd_occupancy_cull_capped on numpy inputs -> (rank, src, pts_live, vd_live | None, (live, kept)) as numpy, every
    output buffer pre-filled with a pattern that no result equals."""
    Rn, S = z.shape
    n, ray_ch = Rn * S, rays.shape[1]
    rt, zt = torch.from_numpy(np.ascontiguousarray(rays)).to(dev), torch.from_numpy(np.ascontiguousarray(z)).to(dev)
    rank = torch.full((max(n, 1),), -7, dtype=torch.int32, device=dev)
    src = torch.full((cap,), -7, dtype=torch.int32, device=dev)
    bc = torch.zeros((n + 255) // 256 + 1, dtype=torch.int32, device=dev)
    pts = torch.full((cap, 3), float("nan"), device=dev)
    vd = torch.full((cap, 3), float("nan"), device=dev) if ray_ch == 11 else None
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    g = grid._c()
    _lib.check(lib.nerf_amd_occupancy_cull_capped(ctypes.byref(g), rt.data_ptr() if Rn else None, ray_ch, zt.data_ptr() if Rn else None,
                                                  Rn, S, cap, bc.data_ptr(), rank.data_ptr(), src.data_ptr(), pts.data_ptr(),
                                                  _lib.ptr(vd), counts.data_ptr(), _lib.stream_of(dev)), "cull_capped")
    torch.cuda.synchronize()
    return (rank[:n].cpu().numpy(), src.cpu().numpy(), pts.cpu().numpy(), None if vd is None else vd.cpu().numpy(),
            tuple(int(v) for v in counts.cpu()), (rank, zt))


def check_cull(dev, grid, rays, z, mask, outside, cap):
    rank, src, pts, vd, counts, keep = run_cull(dev, grid, rays, z, cap)
    e_rank, e_src, e_pts, e_vd, e_counts = T.cull_capped(rays, z, mask, LO, HI, outside == "live", cap)
    assert counts == e_counts, (counts, e_counts)
    assert np.array_equal(rank, e_rank) and np.array_equal(src, e_src)
    assert same_bits(pts, e_pts) and ((vd is None and e_vd is None) or same_bits(vd, e_vd))
    return rank, src, counts, keep


@gpu
@pytest.mark.parametrize("ray_ch", [8, 11])
@pytest.mark.parametrize("outside", ["live", "empty"])
def test_cull_capped_gather_rows_and_ray_grads_equal_their_mirrors(dev, ray_ch, outside):
    rays, mask = H.batch_np(ray_ch), H.half_live_mask()
    grid = grid_of(dev, LO, HI, RES, mask, outside)
    rng = np.random.default_rng(7)
    for z in H.oracle_depths(ray_ch):
        Rn, S = z.shape
        n = Rn * S
        live = T.cull_capped(rays, z, mask, LO, HI, outside == "live", n)[4][0]
        assert n // 4 <= live <= 3 * n // 4
        for cap in (n, live + 37, live, live - 1, live // 2, 1):
            rank, src, counts, (rank_t, z_t) = check_cull(dev, grid, rays, z, mask, outside, cap)
            kept = counts[1]
            assert counts == (live, min(live, cap)) and (src[kept:] == -1).all() and int((rank >= 0).sum()) == kept
            if cap < live:              # the first `cap` live points in point order
                assert np.array_equal(np.nonzero(rank >= 0)[0], np.nonzero(M.cull(rays, z, mask, LO, HI, outside == "live")[0] >= 0)[0][:cap])
            # expand, then its backward: gather_rows(expand(x)) == x on the kept rows, +0.0 on the padding rows
            for ch in (4, 5):
                x = rng.standard_normal((cap, ch)).astype(np.float32)
                xt, src_t = torch.from_numpy(x).to(dev), torch.from_numpy(src).to(dev)
                dense = torch.full((n, ch), float("nan"), device=dev)
                back = torch.full((cap, ch), float("nan"), device=dev)
                _lib.check(lib.nerf_amd_occupancy_expand(xt.data_ptr(), rank_t.data_ptr(), n, ch, dense.data_ptr(), _lib.stream_of(dev)), "expand")
                _lib.check(lib.nerf_amd_occupancy_gather_rows(dense.data_ptr(), src_t.data_ptr(), cap, ch, back.data_ptr(),
                                                              _lib.stream_of(dev)), "gather_rows")
                assert same_bits(dense, T.expand(x, rank)) and same_bits(back, T.gather_rows(T.expand(x, rank), src))
                assert same_bits(back[:kept], x[:kept]) and not back[kept:].any() and not torch.signbit(back[kept:]).any()
            # the backward onto the rays, in the header's order
            g_pts = (rng.standard_normal((cap, 3)) * 10.0 ** rng.integers(-5, 3, (cap, 1))).astype(np.float32)
            g_vd = rng.standard_normal((cap, 3)).astype(np.float32) if ray_ch == 11 else None
            for with_vd in ((True, False) if ray_ch == 11 else (False,)):
                gv = g_vd if with_vd else None
                gp_t, gv_t = torch.from_numpy(g_pts).to(dev), (torch.from_numpy(gv).to(dev) if gv is not None else None)
                out = torch.full((Rn, ray_ch), float("nan"), device=dev)
                _lib.check(lib.nerf_amd_occupancy_ray_grads(rank_t.data_ptr(), z_t.data_ptr(), gp_t.data_ptr(), _lib.ptr(gv_t), Rn, S,
                                                            ray_ch, out.data_ptr(), _lib.stream_of(dev)), "ray_grads")
                assert same_bits(out, T.ray_grads(rank, z, g_pts, gv, ray_ch))


@gpu
def test_cull_capped_edge_shapes(dev):
    """R = 0 (a list that is all padding, counts {0, 0}), S = 1, an all-dead grid, and 200 samples per ray (a lane of the
    ray-gradient wave adds four samples)."""
    rays, mask = H.batch_np(11), H.half_live_mask()
    grid = grid_of(dev, LO, HI, RES, mask, "empty")
    z = H.oracle_depths(11)[1]
    rank, src, counts, _ = check_cull(dev, grid, rays[:0], z[:0], mask, "empty", 5)
    assert counts == (0, 0) and rank.size == 0 and (src == -1).all()
    rank, src, counts, _ = check_cull(dev, grid, rays, np.ascontiguousarray(z[:, 3:4]), mask, "empty", R)           # S = 1
    assert 0 < counts[0] == counts[1] < R
    dead = np.zeros(RES, bool)
    rank, src, counts, _ = check_cull(dev, grid_of(dev, LO, HI, RES, dead, "empty"), rays, z, dead, "empty", 100)
    assert counts == (0, 0) and (rank == -1).all() and (src == -1).all()
    rng = np.random.default_rng(3)
    zz = np.sort(rng.uniform(2, 6, (R, 200)).astype(np.float32), -1)
    rank, src, counts, (rank_t, z_t) = check_cull(dev, grid, rays, zz, mask, "empty", 5000)
    assert counts[1] == 5000 < counts[0]
    g_pts, g_vd = rng.standard_normal((5000, 3)).astype(np.float32), rng.standard_normal((5000, 3)).astype(np.float32)
    out = torch.full((R, 11), float("nan"), device=dev)
    gp_t, gv_t = torch.from_numpy(g_pts).to(dev), torch.from_numpy(g_vd).to(dev)
    _lib.check(lib.nerf_amd_occupancy_ray_grads(rank_t.data_ptr(), z_t.data_ptr(), gp_t.data_ptr(), gv_t.data_ptr(), R, 200, 11,
                                                out.data_ptr(), _lib.stream_of(dev)), "ray_grads")
    assert same_bits(out, T.ray_grads(rank, zz, g_pts, g_vd, 11))


# ================================================================================================ 2. all live = dense
@gpu
@pytest.mark.parametrize("ray_ch", [8, 11])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_all_live_grid_at_fraction_one_is_the_dense_training_call(dev, precision, ray_ch):
    mc, mf = models_of(dev, ray_ch, precision)
    batch = torch.from_numpy(H.batch_np(ray_ch)).to(dev)
    r = renderer(perturb=1.0, use_viewdirs=ray_ch == 11)
    torch.manual_seed(5)
    dense = r.render_rays(batch, mc, mf, retraw=True, retweights=True)
    assert dense["rgb_map"].requires_grad
    cull = occupancy.TrainCull(occupancy.OccupancyGrid([LO, HI], RES, outside="live", device=dev))
    r.train_occupancy = cull
    torch.manual_seed(5)
    got = r.render_rays(batch, mc, mf, retraw=True, retweights=True)
    assert got["rgb_map"].requires_grad and list(got) == list(dense)
    for k in dense:
        assert same_bits(got[k], dense[k]), k
    s = cull.stats()
    assert s["coarse"] == dict(live=R * NC, kept=R * NC, total=R * NC, overflow=0)
    assert s["fine"] == dict(live=R * (NC + NI), kept=R * (NC + NI), total=R * (NC + NI), overflow=0)


# ================================================================================================ 3. half live = the restatement
def restate_pass(r, model, rays, z, mask, outside, cap):
    """One pass from public ops: the mirror's padded list, rebuilt in torch from `rays` (so that autograd reaches them) ->
    model.forward in train mode -> index_put into zeros -> raw [R, S, ch]; also the mirror's counts."""
    dev = rays.device
    Rn, S = z.shape
    rank, src, pts_np, vd_np, counts = T.cull_capped(rays.detach().cpu().numpy(), z.cpu().numpy(), mask, LO, HI, outside == "live", cap)
    src_t = torch.from_numpy(src.astype(np.int64)).to(dev)
    kept = src_t >= 0
    sel = src_t.clamp_min(0)
    ray = sel // S
    pts = rays[ray, 0:3] + rays[ray, 3:6] * z.reshape(-1)[sel][:, None]
    pts = torch.where(kept[:, None], pts, torch.from_numpy(T.centre(LO, HI)).to(dev)[None, :])
    assert same_bits(pts, pts_np)
    vd = None
    if model.use_viewdirs:
        vd = torch.where(kept[:, None], rays[ray, 8:11], torch.tensor([0.0, 0.0, 1.0], device=dev)[None, :])
        assert same_bits(vd, vd_np)
    raw_live = model.forward(pts[:, None, :], vd)[:, 0, :]
    raw = torch.zeros(Rn * S, raw_live.shape[1], device=dev).index_put((src_t[kept],), raw_live[kept])
    return raw.reshape(Rn, S, -1), torch.from_numpy(rank).to(dev), counts


def restate(r, mc, mf, rays, z_c, z_f, mask, outside, fractions=(1.0, 1.0)):
    out, counts = {}, []
    for key, m, z, fr in (("0", mc, z_c, fractions[0]), ("_map", mf, z_f, fractions[1])):
        raw, rank, c = restate_pass(r, m, rays, z, mask, outside, T.capacity(fr, z.numel()))
        rgb, disp, acc, weights, _ = r.raw2outputs(raw, z, rays[:, 3:6])
        out.update({"rgb" + key: rgb, "disp" + key: disp, "acc" + key: acc})
        counts.append(c)
    out.update(raw=raw, weights=weights, rank=rank)
    return out, counts


def coarse_depths(r, batch, mc):
    from nerf_shared_amd import render_utils
    with torch.no_grad():
        one = render_utils.Renderer(**dict(H.CFG, N_importance=0, use_viewdirs=r.use_viewdirs)).render_rays(batch, mc, None, retweights=True)
    return one["z_vals"]


def loss_of(out, target):
    return ((out["rgb_map"] - target) ** 2).mean() + ((out["rgb0"] - target) ** 2).mean()


@gpu
@pytest.mark.parametrize("ray_ch,outside", [(11, "empty"), (8, "live")])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_half_live_grid_equals_the_restatement(dev, precision, ray_ch, outside):
    mask = H.half_live_mask()
    grid = grid_of(dev, LO, HI, RES, mask, outside)
    batch = torch.from_numpy(H.batch_np(ray_ch)).to(dev)
    target = torch.from_numpy(np.random.default_rng(2).uniform(0, 1, (R, 3)).astype(np.float32)).to(dev)
    r = renderer(use_viewdirs=ray_ch == 11)
    mc, mf = models_of(dev, ray_ch, precision)
    z_c = coarse_depths(r, batch, mc)
    cull = occupancy.TrainCull(grid)
    r.train_occupancy = cull
    rays = batch.clone().requires_grad_(True)
    got = r.render_rays(rays, mc, mf, retraw=True, retweights=True)
    loss_of(got, target).backward()
    g_params = [None if p.grad is None else p.grad.clone() for m in (mc, mf) for p in m.parameters()]
    g_rays = rays.grad.clone()
    for m in (mc, mf):
        m.zero_grad()
    r.train_occupancy = None
    rays2 = batch.clone().requires_grad_(True)
    ref, counts = restate(r, mc, mf, rays2, z_c, got["z_vals"].detach(), mask, outside)
    for k in ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "raw", "weights"):
        assert same_bits(got[k], ref[k].reshape(got[k].shape)), k
    culled = ref["rank"].reshape(R, NC + NI) < 0
    assert R * (NC + NI) // 4 <= int(culled.sum()) <= 3 * R * (NC + NI) // 4
    assert not got["raw"][culled].any() and not torch.signbit(got["raw"][culled]).any()          # culled samples: raw == +0.0
    s = cull.stats()
    assert (s["coarse"]["live"], s["coarse"]["kept"]) == counts[0] and (s["fine"]["live"], s["fine"]["kept"]) == counts[1]
    loss_of(ref, target).backward()
    names = [("coarse." if m is mc else "fine.") + n for m in (mc, mf) for n, _ in m.named_parameters()]
    assert sum(g is not None for g in g_params) >= 2 * 2 * 9
    for name, g, p in zip(names, g_params, [p for m in (mc, mf) for p in m.parameters()]):
        if g is None or p.grad is None:     # views_linears of a model without view branch: in nobody's graph
            assert g is None and p.grad is None and "views_linears" in name and ray_ch == 8, name
            continue
        assert g.abs().max() > 0, name
        if "output_linear" in name:         # the head of a model without view branch: float atomics (csrc/backward.hip)
            reordering_gate(g, p.grad)
        else:
            assert same_bits(g, p.grad), (name, float((g - p.grad).abs().max()))
    # the restatement's ray gradients come from torch's index_add (float atomics): the reordering gate
    assert g_rays.shape == rays2.grad.shape and g_rays[:, 0:6].abs().max() > 0 and not g_rays[:, 6:8].any()
    reordering_gate(g_rays, rays2.grad)


@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32_split"])
def test_gradients_of_a_frozen_model_call_reach_the_rays_and_never_the_parameters(dev, precision):
    mask = H.half_live_mask()
    batch = torch.from_numpy(H.batch_np(11)).to(dev)
    target = torch.full((R, 3), 0.5, device=dev)
    r = renderer()
    mc, mf = models_of(dev, 11, precision, train=False)
    z_c = coarse_depths(r, batch, mc)
    r.train_occupancy = occupancy.TrainCull(grid_of(dev, LO, HI, RES, mask, "empty"))
    rays = batch.clone().requires_grad_(True)
    got = r.render_rays(rays, mc, mf, retweights=True)
    loss_of(got, target).backward()
    assert all(p.grad is None for m in (mc, mf) for p in m.parameters())
    r.train_occupancy = None
    rays2 = batch.clone().requires_grad_(True)
    ref, _ = restate(r, mc, mf, rays2, z_c, got["z_vals"].detach(), mask, "empty")
    assert same_bits(got["rgb_map"], ref["rgb_map"]) and same_bits(got["rgb0"], ref["rgb0"])
    loss_of(ref, target).backward()
    assert rays.grad[:, 0:6].abs().max() > 0 and rays.grad[:, 8:11].abs().max() > 0
    reordering_gate(rays.grad, rays2.grad)
    # a frozen model BESIDE a training one keeps its forward-only kernel on the same compact list: no gradient, finite maps
    mf.requires_grad_(True)
    r.train_occupancy = occupancy.TrainCull(grid_of(dev, LO, HI, RES, mask, "empty"))
    out = r.render_rays(batch, mc, mf, retraw=True)
    loss_of(out, target).backward()
    assert all(p.grad is None for p in mc.parameters()) and all(p.grad is not None for p in mf.parameters())
    assert not out["rgb0"].requires_grad and bool(torch.isfinite(out["rgb0"]).all())


# ================================================================================================ 4. the oracle
@gpu
def test_culled_step_gradients_match_fp32_autograd_of_the_oracle_with_the_kept_mask(dev):
    """Precision 'fp32': the culled step's parameter gradients against fp32 autograd of the CPU oracle's two passes with raw
    multiplied by the kept mask (the fine pass on the run's own depths), under the gate tests/test_gpu_train_f32.py applies
    to the dense step (check(..., 1e-3), its reason given there); the figures are printed."""
    from test_gpu_train_f32 import build, check
    arch, mask = P.VD, H.half_live_mask()
    batch = torch.from_numpy(H.batch_np(11))
    target = torch.from_numpy(np.random.default_rng(2).uniform(0, 1, (R, 3)).astype(np.float32))
    mc, cc = build(dev, 1, 3.0, arch)
    mf, cf = build(dev, 19, 3.0, arch)
    r = renderer()
    r.train_occupancy = occupancy.TrainCull(grid_of(dev, LO, HI, RES, mask, "empty"))
    out = r.render_rays(batch.to(dev), mc, mf, retraw=True, retweights=True)
    loss_of(out, target.to(dev)).backward()
    z_f = out["z_vals"].detach().cpu()
    rays_o, rays_d, vd = batch[:, 0:3], batch[:, 3:6], batch[:, 8:11]
    z_c = O.coarse_z_vals(O.RenderCfg(**H.CFG), batch[:, 6:7], batch[:, 7:8], R, None)
    ref = {}
    for key, sd, z in (("rgb0", cc, z_c), ("rgb_map", cf, z_f)):
        pts = rays_o[:, None, :] + rays_d[:, None, :] * z[:, :, None]
        on = M.live(M.lookup(M.ray_points(batch.numpy(), z.numpy()).reshape(-1, 3), LO, HI, RES), mask, False).reshape(z.shape)
        assert 0.25 <= on.mean() <= 0.75
        raw = O.nerf_forward(sd, O.Arch(**arch), pts, vd) * torch.from_numpy(on)[:, :, None].float()
        ref[key] = O.raw2outputs(raw, z, rays_d, True, None)[0]
        if key == "rgb_map":
            print("raw rel-L2 vs the masked oracle: %.2e" % rel_err(out["raw"].detach().cpu(), raw))
            assert rel_err(out["raw"].detach().cpu(), raw) < 1e-5
    loss_of(ref, target).backward()
    print("rgb_map %.2e  rgb0 %.2e" % (rel_err(out["rgb_map"], ref["rgb_map"]), rel_err(out["rgb0"], ref["rgb0"])))
    print("coarse %.2e  fine %.2e" % (check(mc, cc, 1e-3), check(mf, cf, 1e-3)))


# ================================================================================================ 5. overflow
@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32_split"])
def test_overflow_is_a_defined_result(dev, precision):
    mask = H.half_live_mask()
    batch = torch.from_numpy(H.batch_np(11)).to(dev)
    r = renderer()
    mc, mf = models_of(dev, 11, precision)
    z_c = coarse_depths(r, batch, mc)
    cull = occupancy.TrainCull(grid_of(dev, LO, HI, RES, mask, "live"), 0.25, 0.25)
    r.train_occupancy = cull
    got = r.render_rays(batch, mc, mf, retraw=True, retweights=True)
    s = cull.stats(reset=True)
    for name, n in (("coarse", R * NC), ("fine", R * (NC + NI))):
        assert s[name]["total"] == n and s[name]["kept"] == T.capacity(0.25, n) == -(-n // 4)
        assert s[name]["overflow"] == s[name]["live"] - s[name]["kept"] > 0
    assert cull.stats()["fine"] == dict(live=0, kept=0, total=0, overflow=0)
    r.train_occupancy = None
    ref, counts = restate(r, mc, mf, batch, z_c, got["z_vals"].detach(), mask, "live", (0.25, 0.25))
    assert counts == [(s["coarse"]["live"], s["coarse"]["kept"]), (s["fine"]["live"], s["fine"]["kept"])]
    for k in ("rgb_map", "disp_map", "acc_map", "rgb0", "disp0", "acc0", "raw", "weights"):
        assert same_bits(got[k], ref[k].reshape(got[k].shape)), k
    assert int((ref["rank"] >= 0).sum()) == s["fine"]["kept"]
    # calibrate() from exact counts: a few calls at fraction 1.0, then margin * live / total
    cull.coarse_fraction = cull.fine_fraction = 1.0
    r.train_occupancy = cull
    for _ in range(2):
        r.render_rays(batch, mc, mf)
    live = cull.stats()
    fc, ff = cull.calibrate(1.25)
    assert fc == min(1.0, 1.25 * live["coarse"]["live"] / live["coarse"]["total"]) and ff == min(1.0, 1.25 * live["fine"]["live"] / live["fine"]["total"])
    assert 0.25 < fc < 1.0 and 0.25 < ff < 1.0 and cull.stats()["coarse"]["total"] == 0
    r.render_rays(batch, mc, mf)
    s = cull.stats()
    assert s["coarse"]["overflow"] == 0 and s["fine"]["overflow"] == 0 and s["fine"]["kept"] == s["fine"]["live"] > 0


# ================================================================================================ 6. refusals and defaults
@gpu
def test_refusals_and_defaults(dev):
    mask = H.half_live_mask()
    batch = torch.from_numpy(H.batch_np(11)).to(dev)
    mc, mf = models_of(dev, 11, "bf16")
    cull = occupancy.TrainCull(grid_of(dev, LO, HI, RES, mask, "empty"))
    noisy = renderer(raw_noise_std=1.0)
    noisy.train_occupancy = cull
    with pytest.raises(_lib.NerfAmdError, match="raw_noise_std"):
        noisy.render_rays(batch, mc, mf)
    r = renderer(perturb=1.0)
    with torch.no_grad():
        torch.manual_seed(3)
        dense = r.render_rays(batch, mc, mf, retraw=True, retweights=True)
        r.train_occupancy = cull
        torch.manual_seed(3)
        got = r.render_rays(batch, mc, mf, retraw=True, retweights=True)
    assert list(got) == list(dense) and all(same_bits(got[k], dense[k]) for k in dense)          # a no-grad call ignores it
    assert cull.stats()["coarse"]["total"] == 0


# ================================================================================================ 7. captured steps
@gpu
@pytest.mark.parametrize("precision", ["bf16", "fp32_split"])
def test_captured_train_step_culls_and_follows_a_refreshed_grid(dev, precision):
    """utils.CapturedTrainStep with a half-live grid: three replays give the losses of three eager culled steps from the same
    state (perturb 0, as in test_captured_train_step_equals_the_eager_loop, whose gate this is: rtol 2e-5); then
    refresh_from_density re-marks the grid in place -- words.data_ptr() unchanged -- and the next replay equals an eager step
    with the refreshed grid: the captured step reads the grid's bits at replay."""
    from nerf_shared_amd import nerf, optim, utils
    arch = P.VD
    K = synth.lego_intrinsics(400, 400)
    rng = np.random.default_rng(5)
    N, steps = R, 3
    batches = []
    for _ in range(steps + 1):
        idx = rng.choice(160000, size=N, replace=False)
        ro, rd = synth.rays_np(400, 400, K, synth.LEGO_C2W, idx)
        batches.append((torch.from_numpy(np.stack([ro, rd], 0)).to(dev), torch.from_numpy(rng.uniform(0, 1, size=(N, 3)).astype(np.float32)).to(dev)))

    def fresh():
        ms = []
        for seed in (1, 19):
            m = nerf.NeRF(**arch)
            m.load_state_dict(synth.torch_state_dict(seed, 3.0, **{**arch, "skips": tuple(arch["skips"])}))
            m.precision = precision
            ms.append(m.to(dev))
        return ms, optim.Adam(list(ms[0].parameters()) + list(ms[1].parameters()), lr=5e-4, betas=(0.9, 0.999))

    mask_a = torch.from_numpy(H.half_live_mask()).to(dev)
    grid = grid_of(dev, LO, HI, RES, H.half_live_mask(), "empty")
    judge = P.gpu_model(dev, 1, 3.0, precision, **arch)                      # a fixed model the refresh marks the grid from
    cull = occupancy.TrainCull(grid)
    r = renderer()
    r.train_occupancy = cull

    def eager_step(ms, opt, i):
        opt.zero_grad()
        rays, tgt = batches[i]
        rgb, _, _, ex = r.render_from_rays(400, 400, K, 32768, rays, ms[0], ms[1], retraw=True)
        loss = utils.img2mse(rgb, tgt) + utils.img2mse(ex["rgb0"], tgt)
        loss.backward()
        opt.step()
        return float(loss.detach())

    ms, opt = fresh()
    eager = [eager_step(ms, opt, i) for i in range(steps)]
    ptr = grid.words.data_ptr()
    grid.refresh_from_density(judge, threshold=0.0, samples_per_cell=4, dilate=0, seed=3)
    mask_b = grid.mask()
    assert grid.words.data_ptr() == ptr and 0 < int(mask_b.sum()) < grid.n_cells and not torch.equal(mask_b, mask_a)
    pts = grid.sample_points(0, grid.n_cells, 4, 3)
    with torch.no_grad():
        assert torch.equal(mask_b.reshape(-1), (judge.get_density(pts).reshape(-1, 4) > 0).any(1))
    eager.append(eager_step(ms, opt, steps))
    live_b = cull.stats(reset=True)

    grid.set_mask(mask_a)
    assert grid.words.data_ptr() == ptr
    ms2, opt2 = fresh()
    step = utils.CapturedTrainStep(r, 400, 400, K, 32768, ms2[0], ms2[1], opt2, N)
    cull.stats(reset=True)                                                  # (the warm-up steps of the construction count too)
    got = [float(step(*batches[i])) for i in range(steps)]
    grid.refresh_from_density(judge, threshold=0.0, samples_per_cell=4, dilate=0, seed=3)
    assert grid.words.data_ptr() == ptr and torch.equal(grid.mask(), mask_b)
    got.append(float(step(*batches[steps])))
    print("eager   ", ["%.6f" % v for v in eager])
    print("captured", ["%.6f" % v for v in got])
    np.testing.assert_allclose(got, eager, rtol=2e-5)
    s = cull.stats()
    assert s["coarse"] == live_b["coarse"] and 0 < s["fine"]["live"] < s["fine"]["total"] == (steps + 1) * N * (NC + NI) and s["fine"]["overflow"] == 0
    # a slab with another seed, dilated: the undilated plane keeps the other slab's bits, the dilation lands in the same storage
    assert grid.slab(1, 2) == (32, 64)
    grid.refresh_from_density(judge, cells=grid.slab(1, 2), dilate=1, seed=4)
    with torch.no_grad():
        half = (judge.get_density(grid.sample_points(32, 64, 4, 4)).reshape(-1, 4) > 0).any(1)
    raw = torch.cat([mask_b.reshape(-1)[:32], half]).cpu().numpy().reshape(RES)
    assert grid.words.data_ptr() == ptr and np.array_equal(grid.mask().cpu().numpy(), M.dilate(raw, 1))
    assert np.array_equal(grid.raw_words.cpu().numpy(), M.words(raw))


@gpu
@pytest.mark.parametrize("dilate", [0, 1])
def test_refresh_after_a_fill_dilates_what_was_marked_not_what_was_dilated(dev, dilate):
    """fill_from_density then refresh_from_density with the same models, seed and dilation leaves the grid as it was: the
    refresh dilates the fill's undilated marks (a copy of the dilated words would grow the grid by a ring per refresh), in the
    storage the fill left; a refresh of one slab with another seed changes that slab's marks alone."""
    judge = P.gpu_model(dev, 1, 3.0, "bf16", **P.VD)
    grid = occupancy.OccupancyGrid([(-1.5, -0.25, -3.0), (1.0, 0.75, 2.0)], (5, 7, 33), device=dev)        # 1155 cells, 37 words
    grid.fill_from_density(judge, samples_per_cell=4, dilate=dilate, seed=3)
    filled, ptr = grid.mask().cpu().numpy(), grid.words.data_ptr()
    with torch.no_grad():
        marked = (judge.get_density(grid.sample_points(0, grid.n_cells, 4, 3)).reshape(-1, 4) > 0).any(1).cpu().numpy().reshape(grid.resolution)
    assert 0 < marked.sum() < marked.size and np.array_equal(filled, M.dilate(marked, dilate))
    assert dilate == 0 or filled.sum() > marked.sum()
    grid.refresh_from_density(judge, samples_per_cell=4, dilate=dilate, seed=3)
    assert grid.words.data_ptr() == ptr and np.array_equal(grid.mask().cpu().numpy(), filled)
    c0, c1 = grid.slab(1, 3)
    grid.refresh_from_density(judge, cells=(c0, c1), samples_per_cell=4, dilate=dilate, seed=9)
    with torch.no_grad():
        part = (judge.get_density(grid.sample_points(c0, c1, 4, 9)).reshape(-1, 4) > 0).any(1).cpu().numpy()
    expect = marked.reshape(-1).copy()
    expect[c0:c1] = part
    assert not np.array_equal(expect, marked.reshape(-1))
    assert grid.words.data_ptr() == ptr and np.array_equal(grid.mask().cpu().numpy(), M.dilate(expect.reshape(grid.resolution), dilate))


@gpu
def test_it_still_learns(dev):
    """tools/train_demo.py's sphere scene, 600 steps with --occupancy 32 --occupancy-warmup 200 --occupancy-refresh 16 against
    600 dense steps from the same seed: the culled run's test PSNR is no lower than the dense run's minus the spread of the
    dense run over three seeds (measured once by tools/occupancy_train_bench.py --learning and kept, with the PSNRs, in
    profiles/occupancy_train.json), and nothing overflows after the calibration.

    Measured: dense 25.037 dB, culled 24.864 dB, margin 1.010 dB; no overflow (6 648 208 live coarse, 31 869 087 live fine
    samples).  While a refresh still dilated the already dilated grid (see the test above) this test failed on both counts:
    24.023 dB and 16 522 overflowing coarse samples."""
    import json
    import sys
    sys.path.insert(0, os.path.join(P.REPO, "tools"))
    import train_demo
    with open(os.path.join(P.REPO, "profiles", "occupancy_train.json")) as f:
        margin = float(json.load(f)["learning"]["dense_psnr_spread"])
    dense = train_demo.run(steps=600, seed=0, verbose=False)[0]
    culled = train_demo.run(steps=600, seed=0, verbose=False, occupancy_res=32, occupancy_warmup=200, occupancy_refresh=16)[0]
    stats = culled["occupancy"]["stats"]
    print("test PSNR after 600 steps: dense %.3f dB, culled %.3f dB, margin %.3f dB; %s" % (dense["psnr_after"], culled["psnr_after"], margin, stats))
    assert margin > 0 and dense["psnr_after"] > dense["psnr_before"] + 3
    assert culled["psnr_after"] >= dense["psnr_after"] - margin
    for name in ("coarse", "fine"):
        assert stats[name]["overflow"] == 0 and 0 < stats[name]["live"] < stats[name]["total"]


@gpu
def test_captured_pose_step_culls(dev):
    """utils.CapturedPoseStep (frozen models, 64 pixels of a 20 x 20 image) with a half-live grid: three replays against three
    eager culled steps from the same state, under the same gate."""
    from nerf_shared_amd import optim, utils
    import test_gpu_pose_step as S
    Hh = W = 20
    K = synth.lego_intrinsics(Hh, W)
    n, steps = 64, 3
    r = renderer()
    mc, mf = S.frozen_pair(dev, P.VD, "fp32_split", 1.0, seeds=(0, 10))
    with torch.no_grad():
        for m in (mc, mf):
            m.alpha_linear.bias += 1.0
    mc.requires_grad_(False)
    mf.requires_grad_(False)
    pose = torch.from_numpy(S.lego44()).to(dev)
    with torch.no_grad():
        image = r.render_from_pose(Hh, W, K, 32768, pose[:3], mc, mf, retraw=False)[0]
    rng = np.random.default_rng(12)
    batches = []
    for _ in range(steps):
        idx = rng.choice(Hh * W, size=n, replace=False)
        pix = torch.from_numpy(np.stack([idx % W, idx // W], -1)).to(dev)
        batches.append((pix, image[pix[:, 1], pix[:, 0]].contiguous()))
    cull = occupancy.TrainCull(grid_of(dev, LO, HI, RES, H.half_live_mask(), "empty"))
    r.train_occupancy = cull

    def fresh():
        cam = utils.CameraTransf()
        with torch.no_grad():
            for p, p0 in zip(cam.parameters(), [torch.tensor(S.TWIST["w"]), torch.tensor(S.TWIST["v"]), torch.tensor(S.TWIST["theta"])]):
                p.copy_(p0)
        cam = cam.to(dev)
        return cam, optim.Adam(cam.parameters(), lr=0.01, betas=(0.9, 0.999))

    cam, opt = fresh()
    eager = []
    for pix, tgt in batches:
        opt.zero_grad()
        ro, rd = utils.get_rays_at(Hh, W, K, cam(pose), pix)
        rgb = r.render_from_rays(Hh, W, K, 32768, torch.stack([ro, rd], 0), mc, mf, retraw=True)[0]
        loss = utils.img2mse(rgb, tgt)
        loss.backward()
        opt.step()
        eager.append(float(loss.detach()))
    assert all(p.grad is not None and p.grad.abs().max() > 0 for p in cam.parameters())
    live = cull.stats(reset=True)
    assert 0 < live["fine"]["live"] < live["fine"]["total"]
    cam2, opt2 = fresh()
    step = utils.CapturedPoseStep(r, Hh, W, K, 32768, mc, mf, cam2, pose, opt2, n)
    cull.stats(reset=True)
    got = [float(step(*b)) for b in batches]
    print("eager   ", ["%.6e" % v for v in eager])
    print("captured", ["%.6e" % v for v in got])
    np.testing.assert_allclose(got, eager, rtol=2e-5)
    assert all(p.grad is None for m in (mc, mf) for p in m.parameters())
    assert cull.stats()["fine"]["total"] == steps * n * (NC + NI)
