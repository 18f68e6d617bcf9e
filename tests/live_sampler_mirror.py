"""numpy float32 restatement of nerf_amd_occupancy_coarse_z (include/nerf_amd.h, "Occupancy grid"): the reference's
stratified ladder in t mapped through each ray's live probes.  One numpy float32 operation per rounded operation of the
definition, built on tests/occupancy_mirror.py (lookup, live, ray_points) and tests/ray_bounds_mirror.py (probe_depths) --
what the kernel of csrc/occupancy.hip must reproduce bit for bit.  No test lives here; tests/test_live_sampler_host.py and
tests/test_gpu_live_sampler.py import it."""
import numpy as np

import occupancy_mirror as M
import ray_bounds_mirror as B

f32 = np.float32


def probe_bits(rays, mask, lo, hi, outside_live, P):
    """b [R, P] bool: the liveness of the P ray-bounds probes of every ray."""
    rays = np.ascontiguousarray(np.asarray(rays, f32))
    pts = M.ray_points(rays, B.probe_depths(rays, P)).reshape(-1, 3)
    return M.live(M.lookup(pts, lo, hi, np.asarray(mask).shape), mask, outside_live).reshape(rays.shape[0], P)


def pad_bits(b, pad):
    """b' [R, P]: b'_k = OR of b_j over |j - k| <= pad, 0 <= j < P."""
    b = np.asarray(b, bool)
    out = b.copy()
    for d in range(1, min(pad, b.shape[1] - 1) + 1):
        out[:, d:] |= b[:, :-d]
        out[:, :-d] |= b[:, d:]
    return out


def stratified_t(t_vals, t_rand, R):
    """t [R, Nc]: t_vals without jitter; with it lower + (upper - lower) * t_rand between the midpoints of the ladder."""
    t_vals = np.asarray(t_vals, f32)
    if t_rand is None:
        return np.broadcast_to(t_vals, (R, t_vals.shape[0]))
    mids = (f32(0.5) * (t_vals[1:] + t_vals[:-1]).astype(f32)).astype(f32)
    lower, upper = np.concatenate([t_vals[:1], mids]), np.concatenate([mids, t_vals[-1:]])
    return (lower[None] + ((upper - lower).astype(f32)[None] * np.asarray(t_rand, f32)).astype(f32)).astype(f32)


def ladder(rays, t_vals, t_rand=None):
    """z [R, Nc]: what nerf_amd_coarse_z writes (lindisp off): near * (1 - t) + far * t, under perturb jittered in z between
    the midpoints of neighbouring depths."""
    rays, t = np.asarray(rays, f32), np.asarray(t_vals, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        z = ((rays[:, 6:7] * (f32(1) - t)[None]).astype(f32) + (rays[:, 7:8] * t[None]).astype(f32)).astype(f32)
        if t_rand is None:
            return z
        mids = (f32(0.5) * (z[:, 1:] + z[:, :-1]).astype(f32)).astype(f32)
        lower, upper = np.concatenate([z[:, :1], mids], 1), np.concatenate([mids, z[:, -1:]], 1)
        return (lower + ((upper - lower).astype(f32) * np.asarray(t_rand, f32)).astype(f32)).astype(f32)


def warp(bits, near, far, t, P):
    """The warp of step 4 for rows whose padded bits are neither all clear nor all set: (z, e, l_j), each [R, Nc]."""
    bits = np.asarray(bits, bool)
    R, Nc = t.shape
    L = bits.sum(1)
    assert ((L > 0) & (L < P)).all()
    order = np.argsort(~bits, axis=1, kind="stable")                    # the set indices first, ascending
    fl = L.astype(f32)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        w = (far - near).astype(f32)
        a = np.minimum((t * fl).astype(f32), fl)
        j = np.minimum(np.floor(a).astype(np.int64), L[:, None] - 1)
        fr = (a - j.astype(f32)).astype(f32)
        lj = np.take_along_axis(order, j, axis=1)
        e = (lj.astype(f32) + fr).astype(f32)
        u = (e * f32(1.0 / P)).astype(f32)
        assert np.array_equal(u.astype(np.float64) * P, e.astype(np.float64))          # exact: P is a power of two
        z = (near[:, None] + (w[:, None] * u).astype(f32)).astype(f32)
    return z, e, lj


def coarse_depths(rays, mask, lo, hi, outside_live, P, pad, t_vals, t_rand=None, bits=None):
    """(z [R, Nc] float32, L [R] int32, e [R, Nc] float32, l_j [R, Nc] int64) of rays [R, 8|11] on the grid `mask` (bool
    [nx, ny, nz]) over the box lo..hi; e and l_j are 0 in the fallback rows (L == 0 or L == P).  bits [R, P]: the probes'
    liveness given by hand instead of looked up (mask, lo, hi and outside_live are then not read)."""
    rays = np.ascontiguousarray(np.asarray(rays, f32))
    t_vals = np.asarray(t_vals, f32)
    R, Nc = rays.shape[0], t_vals.shape[0]
    b = pad_bits(probe_bits(rays, mask, lo, hi, outside_live, P) if bits is None else bits, pad)
    L = b.sum(1).astype(np.int32)
    z = ladder(rays, t_vals, t_rand)
    e, lj = np.zeros((R, Nc), f32), np.zeros((R, Nc), np.int64)
    rows = np.flatnonzero((L > 0) & (L < P))
    if rows.size:
        t = stratified_t(t_vals, None if t_rand is None else np.asarray(t_rand, f32)[rows], rows.size)
        z[rows], e[rows], lj[rows] = warp(b[rows], rays[rows, 6], rays[rows, 7], t, P)
    return z, L, e, lj
