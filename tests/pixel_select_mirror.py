"""Plain-numpy mirror of the pixel-selection entry points (include/nerf_amd.h: nerf_amd_draw_pixels,
nerf_amd_interest_points, nerf_amd_dilate_mask, nerf_amd_compact_mask), written from their DEFINITIONS, not from the
kernels: the draw is evaluated for all slots at once with array masks, the detector with shifted whole-image arrays, the
dilation literally as I successive passes, the compaction with numpy's boolean indexing.  Everything is integer arithmetic,
so the GPU tests compare for equality."""
import numpy as np


def mix(x):
    """x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16, mod 2^32, on a uint32 array."""
    x = np.asarray(x, dtype=np.uint64)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16))
    return x


def half_bits(M):
    return max(1, (int(M - 1).bit_length() + 1) // 2)


def round_keys(seed, draw):
    """k_r = mix(mix(seed + 0x9e3779b9 (r + 1)) ^ draw), r = 0..3; draw = the low 32 bits of the counter."""
    draw = int(draw) & 0xffffffff
    return [int(mix(int(mix((int(seed) + 0x9e3779b9 * (r + 1)) & 0xffffffff)) ^ draw)) for r in range(4)]


def draw_indices(M, n, seed, draw):
    """perm(0..n-1) of the keyed bijection of [0, M): int64 [n]."""
    assert 1 <= n <= M
    b = np.uint64(half_bits(M))
    mask = np.uint64((1 << int(b)) - 1)
    keys = [np.uint64(k) for k in round_keys(seed, draw)]
    x = np.arange(n, dtype=np.uint64)
    todo = np.ones(n, dtype=bool)
    while todo.any():                                   # the cycle walk: only slots still at or above M take another turn
        cur = x[todo]
        L, R = cur >> b, cur & mask
        for k in keys:
            L, R = R, L ^ (mix(R ^ k) & mask)
        x[todo] = (L << b) | R
        todo = x >= np.uint64(M)
    return x.astype(np.int64)


def draw_pixels(M, n, seed, draw, W=None, region=None):
    """int32 [n, 2] (x, y): the region's entries at the drawn indices, or (i % W, i // W) without a region."""
    idx = draw_indices(M, n, seed, draw)
    if region is not None:
        return np.asarray(region)[idx].astype(np.int32)
    return np.stack([idx % W, idx // W], -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------ detector
def _shift_clamped(a, dy, dx):
    """b[y, x] = a[clamp(y + dy), clamp(x + dx)]."""
    H, W = a.shape
    ys = np.clip(np.arange(H) + dy, 0, H - 1)
    xs = np.clip(np.arange(W) + dx, 0, W - 1)
    return a[ys][:, xs]


def harris_response(image):
    """int64 [H, W]: 25 (Sxx Syy - Sxy^2) - (Sxx + Syy)^2 from the uint8 image [H, W, >= 3]."""
    img = np.asarray(image).astype(np.int64)
    gray = (4899 * img[..., 0] + 9617 * img[..., 1] + 1868 * img[..., 2] + 8192) >> 14
    s = lambda dy, dx: _shift_clamped(gray, dy, dx)          # noqa: E731
    gx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    gy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    sxx, syy, sxy = (np.zeros_like(gray) for _ in range(3))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            u, v = _shift_clamped(gx, dy, dx), _shift_clamped(gy, dy, dx)
            sxx += u * u
            syy += v * v
            sxy += u * v
    return 25 * (sxx * syy - sxy * sxy) - (sxx + syy) ** 2


def interest_mask(image, quality=1):
    """uint8 [H, W]: Rsp > 0, 100 Rsp >= quality max(Rsp), and a 3x3 maximum with ties going to the first in row-major order."""
    r = harris_response(image)
    H, W = r.shape
    on = (r > 0) & (100 * r >= quality * r.max())
    lowest = np.iinfo(np.int64).min
    padded = np.full((H + 2, W + 2), lowest, dtype=np.int64)          # off-image neighbours never win
    padded[1:-1, 1:-1] = r
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            o = padded[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
            inside = o != lowest
            earlier = dy < 0 or (dy == 0 and dx < 0)
            on &= ~inside | ((r > o) if earlier else (r >= o))
    return on.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ dilation, compaction
def dilate(mask, k, iterations):
    """cv2.dilate(mask, ones((k, k)), iterations=I): I passes of out[y, x] = max in[y + dy, x + dx], dy, dx in [-a, k - 1 - a],
    a = k // 2, off-image pixels ignored."""
    cur = np.asarray(mask).astype(np.uint8)
    H, W = cur.shape
    a = k // 2
    for _ in range(iterations):
        out = np.zeros_like(cur)
        for dy in range(-a, k - a):
            for dx in range(-a, k - a):
                y0, y1 = max(0, -dy), min(H, H - dy)
                x0, x1 = max(0, -dx), min(W, W - dx)
                if y0 < y1 and x0 < x1:
                    out[y0:y1, x0:x1] = np.maximum(out[y0:y1, x0:x1], cur[y0 + dy:y1 + dy, x0 + dx:x1 + dx])
        cur = out
    return cur


def compact(mask):
    """coords[mask] of demo_est_rel_pose.py:39-47 with H = mask.shape[0]: int32 [M, 2] (x, y) in row-major order."""
    mask = np.asarray(mask)
    H, W = mask.shape
    coords = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1)
    return coords[mask.astype(bool)].astype(np.int32)


def region_of(image, strategy, kernel_size=5, dil_iter=3, quality=1, points=None):
    """The region list utils.PixelSampler builds: None for 'random'."""
    if strategy == "random":
        return None
    H, W = np.asarray(image).shape[:2]
    if points is None:
        mask = interest_mask(image, quality)
    else:
        mask = np.zeros((H, W), np.uint8)
        pts = np.asarray(points)
        mask[pts[:, 1], pts[:, 0]] = 1
    if strategy == "interest_region":
        mask = dilate(mask, kernel_size, dil_iter)
    return compact(mask)
