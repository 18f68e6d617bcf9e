"""numpy restatements of the capped cull, its row gather and the per-ray gradient reduction (include/nerf_amd.h:
nerf_amd_occupancy_cull_capped, _gather_rows, _ray_grads), on top of tests/occupancy_mirror.py, which stays as it is.  Every
fp32 operation is one numpy float32 operation, in the order the header writes down -- what the kernels of csrc/occupancy.hip
must reproduce bit for bit.  No test lives here; tests/test_train_cull_host.py and tests/test_gpu_train_cull.py import it."""
import math

import numpy as np

import occupancy_mirror as M

f32 = M.f32


def capacity(fraction, n):
    """C = min(n, max(1, ceil(fraction n)))  (occupancy.TrainCull)."""
    return min(n, max(1, int(math.ceil(fraction * n))))


def centre(lo, hi):
    """The point of a padding row: float32((lo + hi) / 2), formed in double from the fp32 box and rounded once."""
    lo, hi = np.asarray(lo, f32).astype(np.float64), np.asarray(hi, f32).astype(np.float64)
    return ((lo + hi) / 2).astype(f32)


def cull_capped(rays, z, mask, lo, hi, outside_live, cap):
    """(rank [R S], src [cap], pts_live [cap, 3], vd_live [cap, 3] | None, (live, kept)): the first `cap` live points in point
    order are kept; rows [kept, cap) are padding: src -1, the box centre, view direction (0, 0, 1)."""
    rays, z = np.asarray(rays, f32), np.asarray(z, f32)
    R, S = z.shape
    has_vd = rays.shape[1] == 11
    src = np.full(cap, -1, np.int32)
    pts_live = np.tile(centre(lo, hi)[None, :], (cap, 1)).astype(f32)
    vd_live = np.tile(np.array([0, 0, 1], f32)[None, :], (cap, 1)) if has_vd else None
    if R == 0:
        return np.zeros(0, np.int32), src, pts_live, vd_live, (0, 0)
    rank, live, pts, vd = M.cull(rays, z, mask, lo, hi, outside_live)
    kept = min(live, cap)
    rank = np.where(rank < cap, rank, -1).astype(np.int32)
    src[:kept] = np.nonzero(rank >= 0)[0]
    pts_live[:kept] = pts[:kept]
    if has_vd:
        vd_live[:kept] = vd[:kept]
    return rank, src, pts_live, vd_live, (live, kept)


def expand(raw_live, rank):
    """raw [n, ch]: row i = raw_live[rank[i]], +0.0 where rank[i] < 0."""
    out = np.zeros((rank.shape[0], raw_live.shape[1]), f32)
    out[rank >= 0] = raw_live[rank[rank >= 0]]
    return out


def gather_rows(dense, src):
    """live [cap, ch]: row i = dense[src[i]], +0.0 where src[i] < 0."""
    out = np.zeros((src.shape[0], dense.shape[1]), f32)
    out[src >= 0] = dense[src[src >= 0]]
    return out


def _reduce64(terms, kept):
    """terms [R, S, k], kept bool [R, S] -> [R, k]: 64 partial sums from +0.0, partial l adds the kept terms of
    s = l, l + 64, ... in ascending order; then v_l = v_l + v_(l xor m) for m = 32, 16, 8, 4, 2, 1."""
    R, S, k = terms.shape
    acc = np.zeros((R, 64, k), f32)
    lanes = np.arange(64)
    for s0 in range(0, S, 64):
        n = min(64, S - s0)
        t = np.zeros((R, 64, k), f32)
        on = np.zeros((R, 64), bool)
        t[:, :n], on[:, :n] = terms[:, s0:s0 + n], kept[:, s0:s0 + n]
        with np.errstate(invalid="ignore", over="ignore"):
            acc = np.where(on[:, :, None], (acc + t).astype(f32), acc)          # a culled sample adds nothing (not even +0.0)
    for m in (32, 16, 8, 4, 2, 1):
        with np.errstate(invalid="ignore", over="ignore"):
            acc = (acc + acc[:, lanes ^ m]).astype(f32)
    return acc[:, 0]


def ray_grads(rank, z, g_pts, g_vd, ray_ch):
    """g_rays [R, ray_ch]: columns 0..2 = sum g_pts, 3..5 = sum (g_pts * z) with the product rounded first, 6..7 = 0,
    8..10 = sum g_vd (0 when g_vd is None); sums over the kept samples of the ray in the header's order."""
    z = np.asarray(z, f32)
    R, S = z.shape
    rank = np.asarray(rank).reshape(R, S)
    kept = rank >= 0
    row = np.maximum(rank, 0)
    gp = np.asarray(g_pts, f32)[row]                                               # [R, S, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        gz = (gp * z[:, :, None]).astype(f32)
    out = np.zeros((R, ray_ch), f32)
    out[:, 0:3], out[:, 3:6] = _reduce64(gp, kept), _reduce64(gz, kept)
    if ray_ch == 11 and g_vd is not None:
        out[:, 8:11] = _reduce64(np.asarray(g_vd, f32)[row], kept)
    return out
