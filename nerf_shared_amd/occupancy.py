"""Occupancy grid: which sample points of a render reach the field kernels (include/nerf_amd.h, "Occupancy grid").

Opt-in.  A grid is a bit per cell of an axis-aligned box in the coordinates the field is evaluated in (after the NDC warp:
NDC coordinates).  It is filled once from the trained models' density and then set on a renderer::

    grid = OccupancyGrid(aabb=[[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]], resolution=128, outside='empty')
    grid.fill_from_density([coarse_model, fine_model])
    renderer.occupancy = grid

Every operation is a HIP kernel of csrc/occupancy.hip with an exactly defined result; there is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import lib

_OUTSIDE = {'live': _lib.OCC_OUTSIDE_LIVE, 'empty': _lib.OCC_OUTSIDE_EMPTY}
MAX_RESOLUTION = 1024
FILL_CHUNK_POINTS = 1 << 20       # points per density launch of fill_from_density (cells per chunk: a multiple of 32)


class OccupancyGrid:
    """aabb: [[lo_x, lo_y, lo_z], [hi_x, hi_y, hi_z]] (or six numbers); resolution: one int or (nx, ny, nz), each 1..1024;
    outside: what a point outside the box is -- 'live' (default, conservative: it is evaluated) or 'empty' (a bounded object);
    device: a ROCm device (default: the current one).  A new grid is all live."""

    def __init__(self, aabb, resolution=128, outside='live', device=None):
        if isinstance(aabb, torch.Tensor):
            aabb = aabb.detach().cpu().numpy()
        try:
            box = np.array(aabb, dtype=np.float32).reshape(-1)          # the box is held in fp32, as the kernels read it
        except (TypeError, ValueError):
            box = np.zeros(0, np.float32)
        if box.size != 6:
            raise ValueError("aabb must hold six numbers: [[lo_x, lo_y, lo_z], [hi_x, hi_y, hi_z]]")
        self.lo, self.hi = [float(v) for v in box[:3]], [float(v) for v in box[3:]]
        if not np.isfinite(box).all() or not all(h > l for l, h in zip(self.lo, self.hi)):
            raise ValueError("aabb must be finite with lo < hi on every axis (got %s .. %s)" % (self.lo, self.hi))
        res = tuple(resolution) if isinstance(resolution, (tuple, list)) else (resolution,) * 3
        if len(res) != 3 or not all(isinstance(n, int) and 1 <= n <= MAX_RESOLUTION for n in res):
            raise ValueError("resolution must be one int or (nx, ny, nz), each 1..%d (got %r)" % (MAX_RESOLUTION, resolution))
        if outside not in _OUTSIDE:
            raise ValueError("outside must be 'live' or 'empty' (got %r)" % (outside,))
        self.resolution, self.outside = res, outside
        self.n_cells = res[0] * res[1] * res[2]
        self.n_words = (self.n_cells + 31) // 32
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if dev.type != 'cuda':
            raise _lib.NerfAmdError("an OccupancyGrid lives on a ROCm (cuda) device, not on %s -- there is no CPU path" % dev)
        self.device = dev
        self._words = None           # made on first use, so building a grid touches no device

    @property
    def words(self):
        """The grid's bits: int32 [(nx ny nz + 31) // 32] on the device, cell c = bit c & 31 of word c >> 5."""
        if self._words is None:
            w = torch.full((self.n_words,), -1, dtype=torch.int32, device=self.device)
            if self.n_cells & 31:
                w[-1] = (1 << (self.n_cells & 31)) - 1          # the unused bits of the last word are 0
            self._words = w
        return self._words

    @words.setter
    def words(self, w):
        self._words = w

    # ------------------------------------------------------------------ plumbing
    def _c(self, words=True):
        g = _lib.OccupancyGridC()
        g.words = self.words.data_ptr() if words else None
        for a in range(3):
            g.lo[a], g.hi[a], g.n[a] = self.lo[a], self.hi[a], self.resolution[a]
        g.outside = _OUTSIDE[self.outside]
        return g

    def _points(self, points, name):
        _lib.require_device(points, name)
        if points.device != self.device:
            raise _lib.NerfAmdError("%s is on %s, the grid on %s" % (name, points.device, self.device))
        if points.dim() < 1 or points.shape[-1] != 3:
            raise _lib.NerfAmdError("%s must be [..., 3], got %s" % (name, tuple(points.shape)))
        return points.detach().reshape(-1, 3).contiguous().float()

    def _lookup(self, points, want_cell):
        pts = self._points(points, "points")
        n = pts.shape[0]
        live = torch.empty(n, dtype=torch.uint8, device=self.device)
        cell = torch.empty(n, dtype=torch.int32, device=self.device) if want_cell else None
        g = self._c()
        with torch.cuda.device(self.device):
            _lib.check(lib.nerf_amd_occupancy_query(ctypes.byref(g), pts.data_ptr(), n, live.data_ptr(), _lib.ptr(cell),
                                                    _lib.stream_of(self.device)), "nerf_amd_occupancy_query")
        return live, cell

    # ------------------------------------------------------------------ queries
    def query(self, points):
        """points [..., 3] -> bool [...]: is the point live (its cell's bit, or the outside policy)."""
        return self._lookup(points, False)[0].bool().reshape(points.shape[:-1])

    def cell_index(self, points):
        """points [..., 3] -> int32 [...]: the linear cell index (ix ny + iy) nz + iz, or -1 outside the box."""
        return self._lookup(points, True)[1].reshape(points.shape[:-1])

    def sample_points(self, c0, c1, samples_per_cell=4, seed=0, out=None):
        """The points the cells [c0, c1) are judged at: [(c1 - c0) samples_per_cell, 3]; sample 0 of a cell is its centre, the
        others a keyed jitter that stays inside the cell (nerf_amd_occupancy_sample_points)."""
        c0, c1, K = int(c0), int(c1), int(samples_per_cell)
        if not (0 <= c0 <= c1 <= self.n_cells) or K < 1:
            raise ValueError("need 0 <= c0 <= c1 <= %d and samples_per_cell >= 1" % self.n_cells)
        n = (c1 - c0) * K
        pts = out[:n] if out is not None else torch.empty(n, 3, dtype=torch.float32, device=self.device)
        g = self._c(words=False)
        with torch.cuda.device(self.device):
            _lib.check(lib.nerf_amd_occupancy_sample_points(ctypes.byref(g), c0, c1, K, int(seed) & 0xffffffff, pts.data_ptr(),
                                                            _lib.stream_of(self.device)), "nerf_amd_occupancy_sample_points")
        return pts

    def mask(self):
        """The grid as bool [nx, ny, nz] (a copy)."""
        shifts = torch.arange(32, dtype=torch.int32, device=self.device)
        bits = (self.words[:, None] >> shifts[None, :]) & 1
        return bits.reshape(-1)[:self.n_cells].bool().reshape(self.resolution)

    def set_mask(self, mask):
        """Replace the grid by bool [nx, ny, nz]."""
        _lib.require_device(mask, "mask")
        if tuple(mask.shape) != self.resolution or mask.device != self.device:
            raise _lib.NerfAmdError("mask must be bool %s on %s (got %s on %s)" % (self.resolution, self.device, tuple(mask.shape), mask.device))
        bits = torch.zeros(self.n_words * 32, dtype=torch.int64, device=self.device)
        bits[:self.n_cells] = mask.reshape(-1).to(torch.int64)
        w = (bits.reshape(-1, 32) << torch.arange(32, dtype=torch.int64, device=self.device)[None, :]).sum(1)
        self.words.copy_(torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32))

    def occupied_fraction(self):
        """Share of live cells.  SYNCHRONISES (the count comes to the host)."""
        return float(self.mask().sum().item()) / self.n_cells

    # ------------------------------------------------------------------ building
    def dilate(self, iterations=1):
        """`iterations` rounds of 3 x 3 x 3 box dilation of the live cells (cells off the grid do not count)."""
        out = torch.empty_like(self.words)
        with torch.cuda.device(self.device):
            _lib.check(lib.nerf_amd_occupancy_dilate(self.words.data_ptr(), self.resolution[0], self.resolution[1], self.resolution[2],
                                                     int(iterations), out.data_ptr(), _lib.stream_of(self.device)),
                       "nerf_amd_occupancy_dilate")
        self.words = out

    def fill_from_density(self, models, threshold=0.0, samples_per_cell=4, dilate=1, seed=0):
        """Set the grid from trained models: a cell is live when any of its `samples_per_cell` sample points has raw
        sigma > threshold in ANY of the models (pass coarse and fine: the grid is the OR of both), then `dilate` rounds of
        dilation.  threshold 0 is the relu cut: a sample with raw sigma <= 0 contributes exactly nothing to a render.
        Each model is evaluated with model.get_density, in its own precision, on the current stream, a chunk of cells at a
        time (one chunk of temporaries alive at a time); nothing synchronises."""
        if not isinstance(models, (list, tuple)):
            models = [models]
        models = [m for m in models if m is not None]
        if not models:
            raise ValueError("fill_from_density needs at least one model")
        K = int(samples_per_cell)
        if K < 1:
            raise ValueError("samples_per_cell must be >= 1")
        cells = max(32, (FILL_CHUNK_POINTS // K) // 32 * 32)
        buf = torch.empty(min(cells, (self.n_cells + 31) // 32 * 32) * K, 3, dtype=torch.float32, device=self.device)
        stream = _lib.stream_of(self.device)
        with torch.no_grad():
            for c0 in range(0, self.n_cells, cells):
                c1 = min(c0 + cells, self.n_cells)
                pts = self.sample_points(c0, c1, K, seed, out=buf)
                for i, m in enumerate(models):
                    sigma = m.get_density(pts).contiguous()
                    with torch.cuda.device(self.device):
                        _lib.check(lib.nerf_amd_occupancy_mark(sigma.data_ptr(), c0, c1, K, float(threshold), int(i > 0),
                                                               self.words.data_ptr(), stream), "nerf_amd_occupancy_mark")
                    del sigma
        if dilate:
            self.dilate(dilate)
        return self
