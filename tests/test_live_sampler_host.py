"""CPU tests of the live-stretch coarse sampler (include/nerf_amd.h, nerf_amd_occupancy_coarse_z): the entry point is bound
with the header's signature and refuses bad grids and arguments before any launch, occupancy.LiveSampler refuses bad probes /
pad, Renderer.coarse_sampler defaults to None -- and the definition, on the mirror (tests/live_sampler_mirror.py), keeps what
the header promises (sorted rows, every sample in a probe interval whose padded bit is set, the range), its fallback rows are
the reference ladder as bits, a scalar restatement of the header's text agrees with the vectorised mirror bit for bit, and the
inputs of tests/test_gpu_live_sampler.py hold misses, all-live, single-stretch and multi-stretch rays in quantity."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

os.environ.setdefault("NERF_AMD_QUIET", "1")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import live_sampler_mirror as S  # noqa: E402
import test_occupancy_host as H  # noqa: E402
import test_train_cull_host as C  # noqa: E402
from nerf_shared_amd import _lib, occupancy, render_utils  # noqa: E402

lib = _lib.lib
NAME = "nerf_amd_occupancy_coarse_z"
f32 = np.float32


def bits_of(a):
    return np.ascontiguousarray(np.asarray(a, f32)).view(np.uint32)


def test_the_symbol_is_bound_with_the_headers_signature():
    with open(os.path.join(REPO, "include", "nerf_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"(int64_t|int)\s+%s\s*\(([^)]*)\)\s*;" % NAME, text)
    assert m, NAME
    args = [H.C_TYPES[re.sub(r"\s*\w+\s*$", "", " ".join(a.split()))] for a in m.group(2).split(",")]      # drop the parameter names
    names = [re.search(r"(\w+)\s*$", a).group(1) for a in m.group(2).split(",")]
    assert names == ["grid", "rays", "ray_ch", "t_vals", "t_rand", "R", "N_samples", "probes", "pad", "lindisp", "perturb", "z_vals",
                     "live_count", "stream"]
    fn = getattr(lib, NAME)
    assert NAME in _lib.EXPORTS
    assert fn.restype is H.C_TYPES[m.group(1)]
    assert list(fn.argtypes) == args, (fn.argtypes, args)
    assert lib.nerf_amd_abi_version() == _lib.ABI_VERSION == 7          # additive: the version stays


def _call(grid=None, rays=1, ray_ch=8, t_vals=2, t_rand=None, R=1, Nc=4, probes=64, pad=1, lindisp=0, perturb=0, z=3, count=4):
    """Pointers are never dereferenced on the host: every call of this file is refused before a launch (or has R == 0)."""
    g = H._grid() if grid is None else grid
    return lib.nerf_amd_occupancy_coarse_z(ctypes.byref(g), rays, ray_ch, t_vals, t_rand, R, Nc, probes, pad, lindisp, perturb, z, count, None)


@pytest.mark.parametrize("bad", [dict(probes=0), dict(probes=63), dict(probes=96), dict(probes=8192), dict(probes=32), dict(probes=-64),
                                 dict(pad=-1), dict(probes=64, pad=65), dict(probes=4096, pad=4097), dict(lindisp=1),
                                 dict(perturb=1), dict(perturb=1, lindisp=1, t_rand=5), dict(z=None), dict(ray_ch=9), dict(ray_ch=3),
                                 dict(R=-1), dict(R=1 << 31), dict(rays=None), dict(t_vals=None), dict(Nc=0)])
def test_bad_arguments_are_refused_before_any_launch(bad):
    assert _call(**bad) == -1
    assert b"occupancy_coarse_z" in lib.nerf_amd_last_error()


@pytest.mark.parametrize("bad", [dict(n=(0, 4, 4)), dict(n=(4, 1025, 4)), dict(lo=(1, -1, -1)), dict(hi=(float("inf"), 1, 1)),
                                 dict(lo=(float("nan"), -1, -1)), dict(outside=2), dict(words=None)])
def test_bad_grids_are_refused_before_any_launch(bad):
    assert _call(grid=H._grid(**bad)) == -1
    assert b"grid" in lib.nerf_amd_last_error()
    assert lib.nerf_amd_occupancy_coarse_z(None, 1, 8, 2, None, 1, 4, 64, 1, 0, 0, 3, 4, None) == -1


def test_no_rays_is_ok_and_launches_nothing():
    assert _call(R=0, rays=None, t_vals=None, z=None, count=None) == 0
    assert _call(R=0, rays=None, pad=64, probes=64, perturb=1) == 0                     # pad == P is fine; no rays, no draws
    for p in (64, 128, 256, 512, 1024, 2048, 4096):
        assert _call(R=0, rays=None, probes=p) == 0
    assert _call(R=0, lindisp=1) == -1                                                  # lindisp is refused whatever R is


def test_live_sampler_refuses_bad_probes_and_pad_and_the_renderer_defaults_to_none():
    g = occupancy.OccupancyGrid([[-1, -1, -1], [1, 1, 1]], 4, device="cuda:0")          # building either touches no device
    for bad in (0, 63, 96, 8192, 32, -64, 256.0, "256", None, True):
        with pytest.raises(ValueError, match="probes"):
            occupancy.LiveSampler(g, probes=bad)
    for bad in (-1, 257, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="pad"):
            occupancy.LiveSampler(g, probes=256, pad=bad)
    with pytest.raises(ValueError, match="pad"):
        occupancy.LiveSampler(g, probes=64, pad=65)
    with pytest.raises(TypeError):
        occupancy.LiveSampler(None)
    with pytest.raises(TypeError):
        occupancy.LiveSampler(occupancy.RayBounds(g))
    ls = occupancy.LiveSampler(g)
    assert (ls.grid, ls.probes, ls.pad) == (g, 256, 1)
    ls = occupancy.LiveSampler(g, 64, 64)
    assert (ls.probes, ls.pad) == (64, 64)
    assert g._words is None                                            # nothing above touched a device
    assert render_utils.Renderer.coarse_sampler is None
    r = render_utils.Renderer(perturb=0.0)
    assert r.coarse_sampler is None and "coarse_sampler" not in r.__dict__ and "coarse_sampler" not in r.state_dict()
    assert r.occupancy is None and r.train_occupancy is None and r.ray_bounds is None


def test_the_training_demo_refuses_a_bad_sampler_before_any_step():
    import sys
    from types import SimpleNamespace
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import train_demo
    r = SimpleNamespace(train_occupancy=1, ray_bounds=1, coarse_sampler=1)
    for probes, pad, what in ((256, 257, "pad"), (256, -1, "pad"), (96, 1, "probes")):
        with pytest.raises(ValueError, match=what):
            train_demo.train_culled(r, None, None, None, 8, 8, None, 64, 16, None, None, 0, 10, train_demo.SPHERE_BOX, 4,
                                    live_sampler_probes=probes, live_sampler_pad=pad)


# ------------------------------------------------------------------------------------------------ the promised invariants
def linspace01(Nc):
    return np.linspace(0.0, 1.0, Nc, dtype=f32)


def hand_rows(P):
    """Live strings set by hand: one live probe at 0, one at P - 1, bits 63 and 64 only (two words, where P has them),
    alternating bits from 0 and from 1."""
    rows = np.zeros((5, P), bool)
    rows[0, 0] = True
    rows[1, P - 1] = True
    rows[2, [63, 64 % P]] = True
    rows[3, 0::2] = True
    rows[4, 1::2] = True
    return rows


def random_rows(rng, R, P):
    return rng.random((R, P)) < rng.choice([0.02, 0.3, 0.9], size=(R, 1))


def near_far_rays(rng, R):
    rays = np.zeros((R, 8), f32)
    rays[:, 6] = rng.uniform(0, 3, R)
    rays[:, 7] = rays[:, 6] + rng.uniform(0.1, 5, R).astype(f32)
    rays[: min(R, 5), 6:8] = [2.0, 6.0]                                # (the hand rows: the interval of the GPU tests)
    return rays


@pytest.mark.parametrize("P", [64, 128, 4096])
def test_the_mirror_keeps_what_the_header_promises(P):
    rng = np.random.default_rng(P)
    warped = beyond_far = 0
    for Nc in (1, 3, 64, 65, 192):
        tv = linspace01(Nc)
        for pad in (0, 1, 64):
            raw = np.concatenate([hand_rows(P), random_rows(rng, 40, P)], 0)
            R = raw.shape[0]
            rays = near_far_rays(rng, R)
            near, far = rays[:, 6], rays[:, 7]
            for t_rand in (None, rng.random((R, Nc), dtype=f32)):
                z, L, e, lj = S.coarse_depths(rays, None, None, None, False, P, pad, tv, t_rand, bits=raw)
                padded = S.pad_bits(raw, pad)
                assert np.array_equal(L, padded.sum(1))
                rows = (L > 0) & (L < P)
                if pad == 0:
                    assert rows[:5].all()                               # every hand row is warped
                warped += int(rows.sum())
                z, e, lj, padded, near_, far_ = z[rows], e[rows], lj[rows], padded[rows], near[rows], far[rows]
                assert (np.diff(z, axis=1) >= 0).all(), (P, Nc, pad)                                    # sorted rows
                assert np.take_along_axis(padded, lj, 1).all()                                          # l_j is a set padded bit
                assert ((e >= lj) & (e <= lj + 1)).all() and ((np.floor(e) == lj) | (e == lj + 1)).all(), (P, Nc, pad)
                top = (near_ + (far_ - near_).astype(f32)).astype(f32)                                  # near (+) (far (-) near)
                assert (z >= near_[:, None]).all() and (z <= top[:, None]).all(), (P, Nc, pad)
                beyond_far += int((z > far_[:, None]).sum())
    print("P = %d: %d warped rows; %d samples beyond far (not promised: the rounding of near + (far - near))" % (P, warped, beyond_far))
    assert warped > 600


def test_hand_rows_land_where_the_text_says():
    """One live probe: every sample lies in that probe's interval.  Bits 63 and 64: two unit intervals side by side across the
    word boundary, the ladder split evenly between them."""
    tv = linspace01(5)
    rays = near_far_rays(np.random.default_rng(0), 5)
    for P in (64, 128, 4096):
        z, L, e, lj = S.coarse_depths(rays, None, None, None, False, P, 0, tv, None, bits=hand_rows(P))
        assert list(L) == [1, 1, 2, P // 2, P // 2]
        assert np.array_equal(e[0], tv) and np.array_equal(e[1], (P - 1) + tv)
        assert z[0, 0] == 2.0 and z[0, -1] == f32(2.0 + 4.0 / P) and z[1, -1] == 6.0
        if P > 64:
            assert np.array_equal(lj[2], [63, 63, 64, 64, 64]) and np.array_equal(e[2], [63, 63.5, 64, 64.5, 65])
        assert np.array_equal(lj[3], [0, P // 4, P // 2, 3 * P // 4, P - 2]) and np.array_equal(lj[4], lj[3] + 1)


# ------------------------------------------------------------------------------------------------ the fallback rows
def reference_ladder(rays, t_vals, t_rand):
    """The reference's own lines (render_utils.py:105-129, lindisp off), in torch on the CPU."""
    near, far = torch.from_numpy(rays[:, 6:7].copy()), torch.from_numpy(rays[:, 7:8].copy())
    z_vals = near * (1. - t_vals) + far * t_vals
    if t_rand is not None:
        mids = .5 * (z_vals[..., 1:] + z_vals[..., :-1])
        upper = torch.cat([mids, z_vals[..., -1:]], -1)
        lower = torch.cat([z_vals[..., :1], mids], -1)
        z_vals = lower + (upper - lower) * torch.from_numpy(t_rand)
    return z_vals.numpy()


@pytest.mark.parametrize("Nc", [1, 3, 64, 65])
def test_miss_and_all_live_rows_are_the_reference_ladder_as_bits(Nc):
    rng = np.random.default_rng(Nc)
    rays = near_far_rays(rng, 12)
    P = 128
    raw = np.zeros((12, P), bool)
    raw[6:] = True                                                      # six misses, six all-live rows
    raw[5, 40] = True                                                   # ... one of the misses becomes all live by its pad
    t_vals = torch.linspace(0., 1., steps=Nc)                          # (the renderer's ladder; numpy's linspace rounds differently)
    for t_rand in (None, rng.random((12, Nc), dtype=f32)):
        z, L, _, _ = S.coarse_depths(rays, None, None, None, False, P, P, t_vals.numpy(), t_rand, bits=raw)
        assert list(L) == [0] * 5 + [P] * 7
        assert np.array_equal(bits_of(z), bits_of(reference_ladder(rays, t_vals, t_rand)))


# ------------------------------------------------------------------------------------------------ the header's text, by hand
def _depths_by_hand(ray, mask, lo, hi, outside_live, P, pad, t_vals, t_rand):
    """The header's definition in scalar float32 operations: plain loops, nothing vectorised, nothing shared with the mirror."""
    f = f32
    n = mask.shape
    lo32, hi32 = [f(v) for v in lo], [f(v) for v in hi]
    scale = [f(n[a] / (float(hi32[a]) - float(lo32[a]))) for a in range(3)]              # formed in double, rounded once
    near, far = f(ray[6]), f(ray[7])
    w = f(far - near)
    b = []
    for k in range(P):                                                                  # 1. the probes
        u = f((k + 0.5) / P)
        t = f(near + f(w * u))
        idx, inside = [], True
        for a in range(3):
            p = f(f(ray[a]) + f(f(ray[3 + a]) * t))
            ta = f(f(p - lo32[a]) * scale[a])
            if not (ta >= 0 and ta < f(n[a])):                                          # false for NaN
                inside = False
                break
            idx.append(int(math.floor(float(ta))))
        b.append(bool(mask[idx[0], idx[1], idx[2]]) if inside else outside_live)
    live = [k for k in range(P) if any(b[j] for j in range(max(k - pad, 0), min(k + pad, P - 1) + 1))]       # 2. the pad
    L, Nc = len(live), len(t_vals)
    tv = [f(v) for v in t_vals]
    z = []
    if L == 0 or L == P:                                                                # 3. the fallback
        zl = [f(f(near * f(f(1) - t)) + f(far * t)) for t in tv]
        for s in range(Nc):
            if t_rand is None:
                z.append(zl[s])
                continue
            lower = f(f(0.5) * f(zl[s] + zl[s - 1])) if s > 0 else zl[s]
            upper = f(f(0.5) * f(zl[s + 1] + zl[s])) if s < Nc - 1 else zl[s]
            z.append(f(lower + f(f(upper - lower) * f(t_rand[s]))))
        return z, L
    for s in range(Nc):                                                                 # 4. the warp
        t = tv[s]
        if t_rand is not None:
            lower = f(f(0.5) * f(tv[s] + tv[s - 1])) if s > 0 else tv[s]
            upper = f(f(0.5) * f(tv[s + 1] + tv[s])) if s < Nc - 1 else tv[s]
            t = f(lower + f(f(upper - lower) * f(t_rand[s])))
        a = min(f(t * f(L)), f(L))
        j = min(int(math.floor(float(a))), L - 1)
        fr = f(a - f(j))
        e = f(f(live[j]) + fr)
        u = f(e * f(1.0 / P))
        z.append(f(near + f(w * u)))
    return z, L


@pytest.mark.parametrize("outside_live", [False, True])
def test_a_scalar_restatement_of_the_header_agrees_with_the_mirror(outside_live):
    rows = [0, 17, 33, 52, 69]
    rays, mask = C.batch_np(11)[rows], C.half_live_mask()
    rng = np.random.default_rng(3)
    seen = set()
    for pad in (0, 1, 64):
        for Nc in (1, 5):
            tv = linspace01(Nc)
            for t_rand in (None, rng.random((len(rows), Nc), dtype=f32)):
                z, L, _, _ = S.coarse_depths(rays, mask, C.LO, C.HI, outside_live, 64, pad, tv, t_rand)
                for r in range(len(rows)):
                    with np.errstate(invalid="ignore"):
                        zh, Lh = _depths_by_hand(rays[r], mask, C.LO, C.HI, outside_live, 64, pad, tv, None if t_rand is None else t_rand[r])
                    assert Lh == L[r]
                    assert np.array_equal(bits_of(zh), bits_of(z[r])), (pad, Nc, r)
                    seen.add("fallback" if Lh in (0, 64) else "warp")
    assert seen == {"fallback", "warp"}


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
def extra_rows(ray_ch, mask, lo, hi, n=40):
    """2 n designed rays behind the batch: n that never come near the box (a miss when the outside is empty, all live when it is
    live) and n that stay inside one live cell (all live either way)."""
    rng = np.random.default_rng(21)
    rows = np.zeros((2 * n, 11), f32)
    rows[:n, 0:3] = 5.0 + rng.random((n, 3))
    rows[:n, 3:6] = rng.uniform(0.1, 1.0, (n, 3))
    cells = np.argwhere(mask)
    cells = cells[rng.integers(0, len(cells), n)]
    rows[n:, 0:3] = np.array(lo) + (cells + 0.5) * (np.array(hi) - np.array(lo)) / np.array(mask.shape)
    rows[n:, 3:6] = rng.uniform(-1e-3, 1e-3, (n, 3))
    rows[:, 6], rows[:, 7] = 2.0, 6.0
    rows[:, 8:11] = rows[:, 3:6] / np.linalg.norm(rows[:, 3:6], axis=1, keepdims=True)
    return np.ascontiguousarray(rows[:, :ray_ch])


def classes(bits):
    """Per row: 'miss', 'all', 'single' (one run of live probes) or 'multi' (at least two separate runs)."""
    bits = np.asarray(bits, bool)
    runs = (bits[:, :1].astype(int) + (bits[:, 1:] & ~bits[:, :-1]).sum(1, keepdims=True))[:, 0]
    L = bits.sum(1)
    return np.where(L == 0, "miss", np.where(L == bits.shape[1], "all", np.where(runs == 1, "single", "multi")))


# (grid, outside, ray_ch, R, P, pad, Nc, perturb): every listed value at least once; the cross-word cases (P = 128, pad 1 and 64)
# with both Nc = 64 and 65
KERNEL_CASES = [
    ("half_live_4", "empty", 11, 259, 64, 0, 64, 0),
    ("half_live_4", "live", 8, 259, 128, 1, 64, 1),
    ("random_8x6x5", "empty", 8, 259, 128, 1, 65, 0),
    ("random_8x6x5", "live", 11, 259, 128, 64, 64, 0),
    ("half_live_4", "empty", 11, 259, 128, 64, 65, 1),
    ("random_8x6x5", "empty", 11, 259, 4096, 3, 192, 1),
    ("half_live_4", "live", 8, 5, 4096, 3, 3, 0),
    ("random_8x6x5", "live", 8, 1, 64, 0, 1, 1),
    ("half_live_4", "empty", 8, 5, 64, 0, 3, 1),
    ("random_8x6x5", "empty", 11, 259, 64, 0, 1, 0),
]


def kernel_inputs(which, ray_ch):
    """(rays [259, ray_ch], mask, resolution): the six edge rows of tests/test_gpu_ray_bounds.py, the 70 rays of the lego view and
    the 80 designed rows, again and again up to 259 rows -- rows [0, R) are R's batch."""
    from test_gpu_occupancy import random_mask
    from test_gpu_ray_bounds import edge_rows
    res, mask = (C.RES, C.half_live_mask()) if which == "half_live_4" else ((8, 6, 5), random_mask((8, 6, 5), 0.3, 4))
    full = np.concatenate([edge_rows(ray_ch, mask, C.LO, C.HI), C.batch_np(ray_ch), extra_rows(ray_ch, mask, C.LO, C.HI)], 0)
    assert full.shape == (156, ray_ch)
    return np.resize(full, (259, ray_ch)), mask, res


def test_gpu_test_inputs_hold_every_class_of_ray():
    count = {"miss": 0, "all": 0, "single": 0, "multi": 0}
    total = 0
    for which, outside, ray_ch, Rn, P, pad, Nc, perturb in KERNEL_CASES:
        rays, mask, _ = kernel_inputs(which, ray_ch)
        with np.errstate(invalid="ignore", over="ignore"):
            padded = S.pad_bits(S.probe_bits(rays[:Rn], mask, C.LO, C.HI, outside == "live", P), pad)
        for c in classes(padded):
            count[c] += 1
        total += Rn
    print(total, "rows:", count)
    for c, n in count.items():
        assert n >= 0.10 * total, (c, n, total)
    for name, values in (("grid", {"half_live_4", "random_8x6x5"}), ("outside", {"live", "empty"}), ("ray_ch", {8, 11}), ("R", {1, 5, 259}),
                         ("P, pad", {(64, 0), (128, 1), (128, 64), (4096, 3)}), ("Nc", {1, 3, 64, 65, 192}), ("perturb", {0, 1})):
        col = {"grid": 0, "outside": 1, "ray_ch": 2, "R": 3, "Nc": 6, "perturb": 7}.get(name)
        got = {(c[4], c[5]) for c in KERNEL_CASES} if col is None else {c[col] for c in KERNEL_CASES}
        assert got == values, name
    for pad in (1, 64):
        assert {c[6] for c in KERNEL_CASES if (c[4], c[5]) == (128, pad)} == {64, 65}
