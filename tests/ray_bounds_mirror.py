"""numpy float32 restatement of nerf_amd_occupancy_ray_bounds (include/nerf_amd.h, "Occupancy grid"): each ray's near / far
clipped to the span over which P probes of it look up live.  One numpy float32 operation per rounded operation of the
definition, built on tests/occupancy_mirror.py (lookup, live, ray_points) -- what the kernel of csrc/occupancy.hip must
reproduce bit for bit.  No test lives here; tests/test_ray_bounds_host.py and tests/test_gpu_ray_bounds.py import it."""
import numpy as np

import occupancy_mirror as M

f32 = np.float32


def probe_depths(rays, P):
    """t [R, P] float32: t_k = near + w * u_k, u_k = (k + 0.5) / P (exact), the product rounded, then the sum."""
    rays = np.asarray(rays, f32)
    near, far = rays[:, 6], rays[:, 7]
    with np.errstate(invalid="ignore", over="ignore"):
        w = (far - near).astype(f32)
        u = ((np.arange(P, dtype=np.float64) + 0.5) / P).astype(f32)
        assert np.array_equal(u.astype(np.float64) * P, np.arange(P) + 0.5)           # exact: P is a power of two
        prod = (w[:, None] * u[None, :]).astype(f32)
        return (near[:, None] + prod).astype(f32)


def ray_bounds(rays, mask, lo, hi, outside_live, P, pad):
    """(rays_out [R, ch], bounds [R, 2] float32, span [R, 2] int32) of rays [R, 8|11] on the grid `mask` (bool [nx, ny, nz])
    over the box lo..hi.  Columns that are copied are copied as bits (a NaN keeps its payload)."""
    rays = np.ascontiguousarray(np.asarray(rays, f32))
    R = rays.shape[0]
    near, far = rays[:, 6], rays[:, 7]
    t = probe_depths(rays, P)
    pts = M.ray_points(rays, t).reshape(-1, 3)
    on = M.live(M.lookup(pts, lo, hi, np.asarray(mask).shape), mask, outside_live).reshape(R, P)
    hit = on.any(1)
    first = np.where(hit, on.argmax(1), -1).astype(np.int64)
    last = np.where(hit, P - 1 - on[:, ::-1].argmax(1), -1).astype(np.int64)
    k0, k1 = np.maximum(first - pad, 0), np.minimum(last + pad, P - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        w = (far - near).astype(f32)
        e0, e1 = (k0 / P).astype(f32), ((k1 + 1) / P).astype(f32)                       # exact
        near2 = (near + (w * e0).astype(f32)).astype(f32)
        far2 = (near + (w * e1).astype(f32)).astype(f32)
    nb, fb = near.view(np.uint32), far.view(np.uint32)
    near2 = np.where(hit & (k0 > 0), near2.view(np.uint32), nb).astype(np.uint32)       # kept ends: the input bits
    far2 = np.where(hit & (k1 < P - 1), far2.view(np.uint32), fb).astype(np.uint32)
    bounds = np.stack([near2, far2], 1).view(f32)
    out = rays.view(np.uint32).copy()
    out[:, 6], out[:, 7] = near2, far2
    return out.view(f32), bounds, np.stack([first, last], 1).astype(np.int32)


def ladder(rays, S):
    """The unperturbed depths of S samples per ray: near * (1 - t) + far * t, t = linspace(0, 1, S) (the coarse ladder of
    render_rays at perturb 0, lindisp off)."""
    rays = np.asarray(rays, f32)
    tt = np.linspace(0, 1, S, dtype=f32)
    return ((rays[:, 6:7] * (f32(1) - tt)[None]).astype(f32) + (rays[:, 7:8] * tt[None]).astype(f32)).astype(f32)
