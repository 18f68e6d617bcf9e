"""Occupancy grid: which sample points of a render reach the field kernels (include/nerf_amd.h, "Occupancy grid").

Opt-in.  A grid is a bit per cell of an axis-aligned box in the coordinates the field is evaluated in (after the NDC warp:
NDC coordinates).  It is filled once from the trained models' density and then set on a renderer::

    grid = OccupancyGrid(aabb=[[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]], resolution=128, outside='empty')
    grid.fill_from_density([coarse_model, fine_model])
    renderer.occupancy = grid

That culls the no-grad render calls.  Training and pose estimation cull through a TrainCull on the same grid
(renderer.train_occupancy = TrainCull(grid)): compact lists of fixed capacity, nothing synchronises, the step still captures;
OccupancyGrid.refresh_from_density keeps the grid following the models in place.

renderer.ray_bounds = RayBounds(grid) moves the samples instead of removing them: every render call first clips each ray's
near / far to the span over which the grid is live along it.

renderer.coarse_sampler = LiveSampler(grid) places the coarse samples instead: the reference's stratified ladder, draw for
draw, mapped through each ray's live probes, so that no coarse sample is spent on the empty stretches of the ray.

Every operation is a HIP kernel of csrc/occupancy.hip with an exactly defined result; there is no CPU path.
"""
import ctypes
import math

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
        self._raw_words = None       # the undilated plane of refresh_from_density, made on its first use

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
        self._raw_words = None       # whoever replaces the grid's bits (dilate, a caller) starts refresh_from_density over

    @property
    def raw_words(self):
        """The undilated plane refresh_from_density marks into: what fill_from_density marked before it dilated, or, for a
        grid that was set another way (set_mask, a caller's words), a copy of `words` made on first use."""
        if self._raw_words is None:
            self._raw_words = self.words.clone()
        return self._raw_words

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

    def _ray_bounds(self, rays, probes, pad, want_rays, want_bounds, want_span):
        """nerf_amd_occupancy_ray_bounds on contiguous fp32 rays [R, 8|11] of this device -> (rays_out, bounds, span), None
        where not asked for.  Enqueue-only."""
        R, dev = rays.shape[0], self.device
        rays_out = torch.empty_like(rays) if want_rays else None
        bounds = torch.empty(R, 2, dtype=torch.float32, device=dev) if want_bounds else None
        span = torch.empty(R, 2, dtype=torch.int32, device=dev) if want_span else None
        g = self._c()
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_occupancy_ray_bounds(ctypes.byref(g), rays.data_ptr(), rays.shape[1], R, int(probes), int(pad),
                                                         _lib.ptr(rays_out), _lib.ptr(bounds), _lib.ptr(span), _lib.stream_of(dev)),
                       "nerf_amd_occupancy_ray_bounds")
        return rays_out, bounds, span

    def _check_rays(self, rays, name="rays"):
        _lib.require_device(rays, name)
        if rays.device != self.device:
            raise _lib.NerfAmdError("%s is on %s, the grid on %s" % (name, rays.device, self.device))
        if rays.dim() != 2 or rays.shape[1] not in (8, 11):
            raise _lib.NerfAmdError("%s must be [N, 8] or [N, 11], got %s" % (name, tuple(rays.shape)))

    def _rays(self, rays, name="rays"):
        self._check_rays(rays, name)
        return rays.detach().contiguous().float()

    def ray_bounds(self, rays, probes=256, pad=1):
        """rays [R, 8|11] -> (bounds [R, 2] float32, span [R, 2] int32): each ray's near / far (columns 6, 7) clipped to the
        span over which `probes` equally spaced probes of it are live, widened by `pad` probe spacings, and the first and
        last live probe ((-1, -1) and the ray's own near / far for a ray with none): nerf_amd_occupancy_ray_bounds.
        probes: a power of two in 64..4096; 0 <= pad <= probes.  Never tracks gradients; nothing synchronises."""
        probes, pad = _probes_pad(probes, pad)
        _, bounds, span = self._ray_bounds(self._rays(rays), probes, pad, False, True, True)
        return bounds, span

    def _coarse_depths(self, rays, t_vals, t_rand, probes, pad, z_out, want_count):
        """nerf_amd_occupancy_coarse_z on contiguous fp32 rays [R, 8|11], t_vals [Nc] and t_rand [R, Nc] | None of this device
        into z_out [R, Nc] (contiguous fp32) -> live_count [R] int32, or None when not asked for.  Enqueue-only."""
        R, dev = rays.shape[0], self.device
        count = torch.empty(R, dtype=torch.int32, device=dev) if want_count else None
        g = self._c()
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_occupancy_coarse_z(ctypes.byref(g), rays.data_ptr(), rays.shape[1], t_vals.data_ptr(), _lib.ptr(t_rand),
                                                       R, t_vals.shape[0], int(probes), int(pad), 0, int(t_rand is not None),
                                                       z_out.data_ptr(), _lib.ptr(count), _lib.stream_of(dev)),
                       "nerf_amd_occupancy_coarse_z")
        return count

    def coarse_depths(self, rays, t_vals, probes=256, pad=1, t_rand=None):
        """rays [R, 8|11], t_vals [Nc] (the ladder in [0, 1]: torch.linspace(0, 1, Nc)) -> (z [R, Nc] float32, live_count [R]
        int32): the stratified ladder mapped through the ray's live probes (`probes` equally spaced probes of [near, far],
        each set one widened by `pad` either way), so that equal steps of t are equal steps of live length; a ray with no
        live probe, or with all of them live, gets the reference ladder: nerf_amd_occupancy_coarse_z.  t_rand [R, Nc] in
        [0, 1): the stratified jitter draws (None: no jitter).  probes: a power of two in 64..4096; 0 <= pad <= probes.
        Never tracks gradients; nothing synchronises."""
        probes, pad = _probes_pad(probes, pad)
        rays = self._rays(rays)
        t_vals = self._floats(t_vals, "t_vals")
        if t_vals.dim() != 1 or t_vals.shape[0] < 1:
            raise _lib.NerfAmdError("t_vals must be [N_samples >= 1], got %s" % (tuple(t_vals.shape),))
        if t_rand is not None:
            t_rand = self._floats(t_rand, "t_rand")
            if tuple(t_rand.shape) != (rays.shape[0], t_vals.shape[0]):
                raise _lib.NerfAmdError("t_rand must be %s, got %s" % ([rays.shape[0], t_vals.shape[0]], tuple(t_rand.shape)))
        z = torch.empty(rays.shape[0], t_vals.shape[0], dtype=torch.float32, device=self.device)
        return z, self._coarse_depths(rays, t_vals, t_rand, probes, pad, z, True)

    def _floats(self, t, name):
        _lib.require_device(t, name)
        if t.device != self.device:
            raise _lib.NerfAmdError("%s is on %s, the grid on %s" % (name, t.device, self.device))
        return t.detach().contiguous().float()

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
        self._raw_words = None

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
        self._mark_cells("fill_from_density", models, 0, self.n_cells, threshold, samples_per_cell, seed, "words")
        self._raw_words = None
        if dilate:
            marked = self._words             # dilate() binds a new tensor to `words`: this one stays the undilated plane, so
            self.dilate(dilate)              # that a later refresh_from_density dilates what was marked, not what was
            self._raw_words = marked         # already dilated
        return self

    def _mark_cells(self, who, models, lo, hi, threshold, samples_per_cell, seed, words):
        """Sets the bits of the cells [lo, hi) of the plane named `words` ('words' / 'raw_words'; lo a multiple of 32) from the
        models' density, a chunk of cells at a time."""
        if not isinstance(models, (list, tuple)):
            models = [models]
        models = [m for m in models if m is not None]
        if not models:
            raise ValueError("%s needs at least one model" % who)
        K = int(samples_per_cell)
        if K < 1:
            raise ValueError("samples_per_cell must be >= 1")
        cells = max(32, (FILL_CHUNK_POINTS // K) // 32 * 32)
        buf = torch.empty(min(cells, (hi - lo + 31) // 32 * 32) * K, 3, dtype=torch.float32, device=self.device)
        stream = _lib.stream_of(self.device)
        words = getattr(self, words)
        with torch.no_grad():
            for c0 in range(lo, hi, cells):
                c1 = min(c0 + cells, hi)
                pts = self.sample_points(c0, c1, K, seed, out=buf)
                for i, m in enumerate(models):
                    sigma = m.get_density(pts).contiguous()
                    with torch.cuda.device(self.device):
                        _lib.check(lib.nerf_amd_occupancy_mark(sigma.data_ptr(), c0, c1, K, float(threshold), int(i > 0),
                                                               words.data_ptr(), stream), "nerf_amd_occupancy_mark")
                    del sigma

    def refresh_from_density(self, models, cells=None, threshold=0.0, samples_per_cell=4, dilate=1, seed=0):
        """Follow the models while they train: re-mark the cells [c0, c1) = `cells` (default: every cell) as fill_from_density
        marks them, into the separate undilated plane `raw_words` (fill_from_density's marks before its dilation; for a grid
        set another way a copy of `words` made on first use -- use the `dilate` the grid was filled with), then dilate
        `raw_words` INTO the existing `words` storage.  `words` is never rebound -- a captured step has baked
        words.data_ptr(), and reads the grid's bits at replay -- and nothing synchronises: every launch is enqueued on the
        current stream, so call it between replays on the stream that replays.  c0 must be a multiple of 32 and c1 a
        multiple of 32 or the number of cells (a marking thread owns whole words).  A rotating slab with a changing seed is
        the caller's loop -- "every k steps refresh 1/m of the cells"::

            if step % k == 0:
                i = (step // k) % m
                grid.refresh_from_density(models, cells=grid.slab(i, m), seed=step)
        """
        c0, c1 = (0, self.n_cells) if cells is None else (int(cells[0]), int(cells[1]))
        if not (0 <= c0 <= c1 <= self.n_cells) or c0 % 32 or (c1 % 32 and c1 != self.n_cells):
            raise ValueError("cells must be (c0, c1) with 0 <= c0 <= c1 <= %d, c0 a multiple of 32 and c1 a multiple of 32 or "
                             "the number of cells (got %r)" % (self.n_cells, cells))
        self._mark_cells("refresh_from_density", models, c0, c1, threshold, samples_per_cell, seed, "raw_words")
        raw = self.raw_words
        with torch.cuda.device(self.device):
            _lib.check(lib.nerf_amd_occupancy_dilate(raw.data_ptr(), self.resolution[0], self.resolution[1], self.resolution[2],
                                                     int(dilate), self._words.data_ptr(), _lib.stream_of(self.device)),
                       "nerf_amd_occupancy_dilate")
        return self

    def slab(self, i, m):
        """The i-th (mod m) of m contiguous cell ranges that cover the grid, each starting at a multiple of 32."""
        per = (self.n_words + m - 1) // m * 32
        c0 = min((i % m) * per, self.n_cells)
        return c0, min(c0 + per, self.n_cells)


MIN_PROBES, MAX_PROBES = 64, 4096


def _probes_pad(probes, pad):
    """The two as ints, or ValueError: probes a power of two in 64..4096, 0 <= pad <= probes."""
    if isinstance(probes, bool) or not isinstance(probes, int) or not (MIN_PROBES <= probes <= MAX_PROBES) or probes & (probes - 1):
        raise ValueError("probes must be a power of two in %d..%d (got %r)" % (MIN_PROBES, MAX_PROBES, probes))
    if isinstance(pad, bool) or not isinstance(pad, int) or not (0 <= pad <= probes):
        raise ValueError("pad must be an int in 0..probes (got %r)" % (pad,))
    return probes, pad


class RayBounds:
    """Clips each ray's near / far to the span over which the grid is live along it (set it as Renderer.ray_bounds): all
    N_samples coarse samples, and the fine samples drawn from them, then lie where the scene is.  Every public render entry
    applies it exactly once per call, to the batch as a whole, before its chunk loop and before any draw; it composes with
    Renderer.occupancy and Renderer.train_occupancy (which still remove the gaps inside the span; the grids may differ).
    The kernel is enqueue-only and reads the grid's words when it runs, so a captured step contains it and follows
    OccupancyGrid.refresh_from_density.  Clipping is not idempotent -- a second clip probes the narrowed interval -- so do
    not apply it to a batch that a renderer will clip again.  Building one touches no device.

    TRAINING needs a wide pad.  The default pad = 1 is meant for rendering a trained model (measured: no loss).  Training
    the sphere scene of tools/train_demo.py with it -- and with pad 8 -- ended 2.4 dB below the dense run; at pad 32 of 256
    probes it ended level with it (profiles/occupancy_bounds.json).  tools/train_demo.py trains at 32."""

    def __init__(self, grid, probes=256, pad=1):
        if not isinstance(grid, OccupancyGrid):
            raise TypeError("grid must be an OccupancyGrid (got %s)" % type(grid).__name__)
        self.grid = grid
        self.probes, self.pad = _probes_pad(probes, pad)

    def apply(self, rays):
        """rays [R, 8|11] -> the batch with columns 6, 7 clipped (fp32, contiguous).  For a batch that requires grad the
        result carries the gradient of every other column back; the bounds are constants of the step (columns 6, 7 get +0.0),
        as z_samples.detach() is in the reference."""
        if rays.is_cuda and rays.device != self.grid.device:
            raise _lib.NerfAmdError("Renderer.ray_bounds is on %s, the rays on %s" % (self.grid.device, rays.device))
        if torch.is_grad_enabled() and rays.requires_grad:
            self.grid._check_rays(rays)                                # (the conversion below is autograd's)
            return _RayBoundsFn.apply(rays.contiguous().float(), self)
        return self.grid._ray_bounds(self.grid._rays(rays), self.probes, self.pad, True, False, False)[0]


class LiveSampler:
    """Places each ray's coarse samples in its live stretches (set it as Renderer.coarse_sampler): every render path asks it
    for the coarse depths instead of nerf_amd_coarse_z.  The reference's stratified ladder in t is kept, draw for draw --
    the same t_rand of the same shape from the same generator -- and mapped through the ray's live probes
    (OccupancyGrid.coarse_depths), so equal steps of t are equal steps of live length; a ray that misses the grid, or whose
    probes are all live, keeps the reference ladder bit for bit, so an all-live grid changes nothing.  Hierarchical
    resampling, compositing and the culls are untouched; the depths are constants of the step, as they always were.  It
    composes with Renderer.occupancy, Renderer.train_occupancy and Renderer.ray_bounds (the batch is clipped first and the
    clipped interval is probed).  lindisp is refused.  The kernel is enqueue-only and reads the grid's words when it runs,
    so a captured step contains it and follows a grid changed in place.  Building one touches no device.

    The depths SPAN the gaps: a sample with sigma > 0 at the end of a stretch is composited over the whole gap behind it,
    and the bins of the resampling can span a gap (fine samples landing there are dropped by the culls when set, evaluated
    otherwise).

    MEASURED on the trained sphere scene (tools/occupancy_sampler_bench.py, profiles/occupancy_sampler.json, DESIGN.md section
    8e.3; 256 probes, pad 1, a culled 400 x 400 view): the kernel takes 0.084 ms for 160 000 rays.  92 % of the coarse samples
    of the rays that hit the grid look up live, against 31 % of the reference ladder -- and 91 % with RayBounds alone: a ray
    through that scene has one live stretch, so there are no inner gaps to drop and the sampler does what the bounds do.  At
    64 + 128 the view is 0.36 dB closer to the ground truth and SLOWER (14.0 against 9.1 ms: three times as many coarse samples
    survive the cull); at 32 + 64 it takes 7.4 ms and is 0.29 dB closer than the 64 + 128 culled view, at 16 + 32 4.0 ms (0.44 x)
    and 0.04 dB further.
    TRAINING with it loses quality: 600 steps of tools/train_demo.py end 4.2 dB below the dense run at pad 1, 1.5 dB at pad 8
    and 1.0 dB at pad 32 -- the whole of the dense run's 1.01 dB spread between seeds.  tools/train_demo.py therefore leaves
    it off (--live-sampler P turns it on), and no test claims that it still learns."""

    def __init__(self, grid, probes=256, pad=1):
        if not isinstance(grid, OccupancyGrid):
            raise TypeError("grid must be an OccupancyGrid (got %s)" % type(grid).__name__)
        self.grid = grid
        self.probes, self.pad = _probes_pad(probes, pad)

    def fill(self, rays, t_vals, t_rand, z_out):
        """The coarse depths of contiguous fp32 rays [R, 8|11] into z_out [R, Nc] (t_rand [R, Nc] | None: the jitter draws)."""
        if rays.device != self.grid.device:
            raise _lib.NerfAmdError("Renderer.coarse_sampler is on %s, the rays on %s" % (self.grid.device, rays.device))
        self.grid._coarse_depths(rays, t_vals, t_rand, self.probes, self.pad, z_out, False)


class _RayBoundsFn(torch.autograd.Function):
    """nerf_amd_occupancy_ray_bounds on the detached batch (contiguous fp32: RayBounds.apply converts, so that autograd
    handles the dtype); the backward passes the gradient on with columns 6, 7 = +0.0."""

    @staticmethod
    def forward(ctx, rays, rb):
        return rb.grid._ray_bounds(rays.detach(), rb.probes, rb.pad, True, False, False)[0]

    @staticmethod
    def backward(ctx, g):
        g = g.clone()
        g[:, 6:8] = 0.0
        return g, None


def _capacity(fraction, n):
    """C = min(n, max(1, ceil(fraction n)))."""
    return min(n, max(1, int(math.ceil(fraction * n)))) if n > 0 else 1


class TrainCull:
    """The occupancy grid in training and pose estimation (set it as Renderer.train_occupancy): every pass of a "train"
    call compacts its live sample points into a list of FIXED capacity C = min(R S, max(1, ceil(fraction R S))), the
    training kernels run on that list in their explicit-points mode (R = C, S = 1), and nothing synchronises, so the step
    can be captured (utils.CapturedTrainStep and the pose steps capture whatever the renderer does: the fractions are
    frozen at capture, the grid's bits are read at replay).  Rows past the live count are padding (the box centre, a zero
    dL/draw row); live points past the cap OVERFLOW: they are treated as empty -- raw = +0.0, no gradient -- which is a
    defined result, visible in stats(), never an error.

    The caller drives the calibration: a few eager steps at fraction 1.0 (no saving, but the counts are exact), then
    calibrate(), then capture::

        cull = occupancy.TrainCull(grid)
        renderer.train_occupancy = cull
        for _ in range(8): eager_step()
        cull.calibrate(margin=1.25)
        step = utils.CapturedTrainStep(...)
        cull.stats(reset=True)            # the warm-up steps of the construction counted too

    Keep the eager steps in a function of their own: a render result that outlives them keeps an autograd graph over the
    parameters alive into the capture (utils.CapturedTrainStep).
    """

    PASSES = ("coarse", "fine")

    def __init__(self, grid, coarse_fraction=1.0, fine_fraction=1.0):
        if not isinstance(grid, OccupancyGrid):
            raise TypeError("grid must be an OccupancyGrid (got %s)" % type(grid).__name__)
        self.grid = grid
        self.coarse_fraction = self._fraction(coarse_fraction, "coarse_fraction")
        self.fine_fraction = self._fraction(fine_fraction, "fine_fraction")
        self._totals = None          # int64 [2, 3] on the grid's device: {live, kept, total} per pass; made on first use

    @staticmethod
    def _fraction(v, name):
        try:
            f = float(v)
        except (TypeError, ValueError):
            f = float("nan")
        if not (0.0 < f <= 1.0):
            raise ValueError("%s must be in (0, 1] (got %r)" % (name, v))
        return f

    def capacity(self, fine_pass, n_points):
        return _capacity(self.fine_fraction if fine_pass else self.coarse_fraction, int(n_points))

    @property
    def totals(self):
        if self._totals is None:
            self._totals = torch.zeros(2, 3, dtype=torch.int64, device=self.grid.device)
        return self._totals

    def cull(self, rays, z, fine_pass):
        """rays [R, 8|11], z [R, S] (fp32, contiguous, on the grid's device) -> (pts_live [C, 3], vd_live [C, 3] | None, rank
        [R S], src [C]); differentiable with respect to the rays.  Adds the pass's counts to the running totals (a torch add
        on the current stream: it captures)."""
        if rays.device != self.grid.device:
            raise _lib.NerfAmdError("Renderer.train_occupancy is on %s, the rays on %s" % (self.grid.device, rays.device))
        return _CullFn.apply(rays, z, self, bool(fine_pass))

    def stats(self, reset=False):
        """{'coarse': {live, kept, total, overflow}, 'fine': {...}} since the last reset, overflow = live - kept.
        SYNCHRONISES: the totals come to the host."""
        t = self.totals.cpu().tolist()
        if reset:
            self.totals.zero_()
        return {name: dict(live=row[0], kept=row[1], total=row[2], overflow=row[0] - row[1]) for name, row in zip(self.PASSES, t)}

    def calibrate(self, margin=1.25):
        """Set each pass's fraction to min(1, margin live / total) from the totals gathered so far (a pass that has not run
        keeps its fraction) and reset them.  SYNCHRONISES (stats).  Returns the two fractions."""
        if not margin >= 1.0:
            raise ValueError("margin must be >= 1 (got %r)" % (margin,))
        s = self.stats(reset=True)
        for name in self.PASSES:
            if s[name]["total"] > 0:
                f = min(1.0, margin * s[name]["live"] / s[name]["total"])
                setattr(self, name + "_fraction", f if f > 0.0 else 1.0 / s[name]["total"])
        return self.coarse_fraction, self.fine_fraction


class _CullFn(torch.autograd.Function):
    """nerf_amd_occupancy_cull_capped; the backward (it runs only when the rays require a gradient) is
    nerf_amd_occupancy_ray_grads."""

    @staticmethod
    def forward(ctx, rays, z, cull, fine_pass):
        grid, dev = cull.grid, rays.device
        R, S = z.shape
        n = R * S
        C = cull.capacity(fine_pass, n)
        has_vd = rays.shape[1] == 11
        f = dict(device=dev, dtype=torch.float32)
        i32 = dict(device=dev, dtype=torch.int32)
        rank, src = torch.empty(n, **i32), torch.empty(C, **i32)
        block_counts = torch.empty((n + 255) // 256, **i32)
        pts, vd = torch.empty(C, 3, **f), (torch.empty(C, 3, **f) if has_vd else None)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        g = grid._c()
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_occupancy_cull_capped(ctypes.byref(g), rays.data_ptr(), rays.shape[1], z.data_ptr(), R, S, C,
                                                          block_counts.data_ptr(), rank.data_ptr(), src.data_ptr(), pts.data_ptr(),
                                                          _lib.ptr(vd), counts.data_ptr(), _lib.stream_of(dev)),
                       "nerf_amd_occupancy_cull_capped")
        row = cull.totals[1 if fine_pass else 0]
        row[:2].add_(counts)
        row[2].add_(n)
        ctx.save_for_backward(rank, z)
        ctx.ray_ch = rays.shape[1]
        ctx.mark_non_differentiable(rank, src)
        ctx.set_materialize_grads(False)
        return pts, vd, rank, src

    @staticmethod
    def backward(ctx, g_pts, g_vd, _g_rank, _g_src):
        if g_pts is None and g_vd is None:
            return None, None, None, None
        rank, z = ctx.saved_tensors
        R, S = z.shape
        dev = z.device
        if g_pts is None:
            g_pts = torch.zeros(g_vd.shape[0], 3, device=dev, dtype=torch.float32)
        g_pts = g_pts.contiguous().float()
        g_vd = None if g_vd is None else g_vd.contiguous().float()
        g_rays = torch.empty(R, ctx.ray_ch, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_occupancy_ray_grads(rank.data_ptr(), z.data_ptr(), g_pts.data_ptr(), _lib.ptr(g_vd), R, S, ctx.ray_ch,
                                                        g_rays.data_ptr(), _lib.stream_of(dev)), "nerf_amd_occupancy_ray_grads")
        return g_rays, None, None, None


class _ExpandFn(torch.autograd.Function):
    """raw_live [C, ch] -> raw [n, ch] (nerf_amd_occupancy_expand: +0.0 where rank < 0); the backward is
    nerf_amd_occupancy_gather_rows (+0.0 in the padding rows)."""

    @staticmethod
    def forward(ctx, raw_live, rank, src):
        raw_live = raw_live.contiguous()
        n, ch, dev = rank.shape[0], raw_live.shape[1], raw_live.device
        raw = torch.empty(n, ch, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_occupancy_expand(raw_live.data_ptr(), rank.data_ptr(), n, ch, raw.data_ptr(), _lib.stream_of(dev)),
                       "nerf_amd_occupancy_expand")
        ctx.save_for_backward(src)
        ctx.ch = ch
        return raw

    @staticmethod
    def backward(ctx, g_raw):
        src, = ctx.saved_tensors
        g = g_raw.contiguous().float()
        dev = g.device
        g_live = torch.empty(src.shape[0], ctx.ch, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_occupancy_gather_rows(g.data_ptr(), src.data_ptr(), src.shape[0], ctx.ch, g_live.data_ptr(),
                                                          _lib.stream_of(dev)), "nerf_amd_occupancy_gather_rows")
        return g_live, None, None
