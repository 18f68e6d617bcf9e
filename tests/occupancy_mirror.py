"""numpy float32 / uint32 restatements of the occupancy grid's definitions (include/nerf_amd.h, "Occupancy grid"): the lookup,
the keyed jitter of the sample points, the dilation and the per-view compaction.  Every fp32 operation is one numpy float32
operation (rounded once), every integer operation uint32 mod 2^32 -- what the kernels of csrc/occupancy.hip must reproduce
bit for bit.  No test lives here; tests/test_occupancy_host.py and tests/test_gpu_occupancy.py import it."""
import numpy as np

f32 = np.float32


def geometry(lo, hi, n):
    """(lo, scale, width, n): scale = float32(n / (hi - lo)), width = float32((hi - lo) / n), formed in double, rounded once."""
    lo, hi = np.asarray(lo, f32), np.asarray(hi, f32)
    n = np.asarray(n, np.int64)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    return lo, (n / ext).astype(f32), (ext / n).astype(f32), n


def lookup(pts, lo, hi, n):
    """Linear cell index of pts [N,3] (float32), -1 outside: t = (p - lo) * scale, two rounded operations per axis."""
    lo, scale, _, n = geometry(lo, hi, n)
    pts = np.asarray(pts, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (pts - lo[None, :]).astype(f32) * scale[None, :]
        assert t.dtype == f32
        inside = np.all((t >= 0) & (t < n[None, :].astype(f32)), axis=1)         # false for NaN
        i = np.floor(np.where(inside[:, None], t, 0)).astype(np.int64)
    c = (i[:, 0] * n[1] + i[:, 1]) * n[2] + i[:, 2]
    return np.where(inside, c, -1).astype(np.int32)


def live(cell, mask, outside_live):
    """mask: bool [nx, ny, nz]; cell from lookup()."""
    flat = np.asarray(mask, bool).reshape(-1)
    return np.where(cell >= 0, flat[np.maximum(cell, 0)], bool(outside_live))


def words(mask):
    """The int32 words of a bool [nx, ny, nz] mask: cell c is bit c & 31 of word c >> 5, unused bits 0."""
    flat = np.asarray(mask, bool).reshape(-1)
    bits = np.zeros((flat.size + 31) // 32 * 32, np.uint32)
    bits[:flat.size] = flat
    w = (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint32)[None, :]).sum(1, dtype=np.uint64).astype(np.uint32)
    return w.view(np.int32)


def mix(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d); x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b); x ^= x >> np.uint32(16)
    return x


def sample_points(lo, hi, n, c0, c1, K, seed):
    """[(c1 - c0) K, 3] float32: sample 0 the cell centre, sample j >= 1 at the 8-bit lattice offsets of
    h = mix(mix(seed + 0x9e3779b9 j) ^ c);  p = lo + (i + f) * width, two rounded operations."""
    lo, _, width, n = geometry(lo, hi, n)
    c = np.repeat(np.arange(c0, c1, dtype=np.uint32), K)
    j = np.tile(np.arange(K, dtype=np.uint32), c1 - c0)
    with np.errstate(over="ignore"):
        h = mix(mix(np.uint32(seed) + np.uint32(0x9e3779b9) * j) ^ c)
    hb = np.stack([h & 255, (h >> 8) & 255, (h >> 16) & 255], 1).astype(f32)
    f = np.where((j > 0)[:, None], (hb + f32(0.5)) * f32(1.0 / 256.0), f32(0.5)).astype(f32)
    cc = c.astype(np.int64)
    i = np.stack([cc // (n[2] * n[1]), (cc // n[2]) % n[1], cc % n[2]], 1).astype(f32)
    u = ((i + f).astype(f32) * width[None, :]).astype(f32)
    return (lo[None, :] + u).astype(f32)


def dilate(mask, iterations):
    """`iterations` rounds of: a cell is set when any of its 27 neighbours (itself included) is; off-grid cells do not count."""
    m = np.asarray(mask, bool)
    for _ in range(iterations):
        p = np.pad(m, 1)
        out = np.zeros_like(m)
        for dx in range(3):
            for dy in range(3):
                for dz in range(3):
                    out |= p[dx:dx + m.shape[0], dy:dy + m.shape[1], dz:dz + m.shape[2]]
        m = out
    return m


def ray_points(rays, z):
    """[R, S, 3] float32: o + d * z, the product rounded before the sum (the field kernels' rays + z_vals mode)."""
    rays, z = np.asarray(rays, f32), np.asarray(z, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (rays[:, None, 3:6] * z[:, :, None]).astype(f32)
        return (rays[:, None, 0:3] + prod).astype(f32)


def cull(rays, z, mask, lo, hi, outside_live):
    """(rank [R S] int32, count, pts_live [count, 3], vd_live [count, 3] or None) of rays [R, 8|11] at depths z [R, S]."""
    pts = ray_points(rays, z).reshape(-1, 3)
    on = live(lookup(pts, lo, hi, np.asarray(mask).shape), mask, outside_live)
    rank = np.where(on, np.cumsum(on) - 1, -1).astype(np.int32)
    vd = None
    if rays.shape[1] == 11:
        vd = np.repeat(np.asarray(rays, f32)[:, 8:11], z.shape[1], axis=0)[on]
    return rank, int(on.sum()), pts[on], vd
