"""Drop-in for nerf_shared/render_utils.py: the volumetric Renderer, running on
the MI355X kernels behind include/nerf_amd.h.

Same constructor, methods, argument names, return structures and key order as
/root/reference/nerf_shared/render_utils.py:13-319.  Differences, all at the
edges of the hot path:
  * temporaries are allocated on ``ray_batch.device`` (the reference uses the
    process-wide default device, main.py:150-152);
  * random draws use torch's generator for that device in the reference's order
    and shapes -- per render_rays call, i.e. per chunk of render_batch: t_rand,
    coarse noise, u, fine noise (render_utils.py:121,264, utils.py:86) -- so a
    seeded multi-chunk render equals seeded per-chunk render_rays calls in every
    mode of render_batch; ``pytest=True`` reproduces the reference's seeded numpy
    draws bit for bit;
  * the NaN/Inf scan of every output (render_utils.py:170-172) only runs when
    DEBUG is set -- it never changes outputs and costs a device sync per key;
  * autograd reaches the models' parameters and the rays (standard model, bf16 mode).
"""
import collections
import ctypes
import os

import numpy as np
import torch

from . import _lib, utils
from . import nerf as nerf_mod
from ._lib import lib
from .nerf import NeRF

DEBUG = False

_KEYS_MAIN = ('rgb_map', 'disp_map', 'acc_map')
_IO_OUT_KEYS = ('rgb_map', 'disp_map', 'acc_map', 'rgb0', 'disp0', 'acc0', 'z_std', 'raw', 'weights', 'z_vals')      # nerf_amd_render_io's outputs

# The random draws of one render_rays call, in the reference's order (Renderer._draws).  A field is None where the reference
# draws nothing; t_lin is the deterministic u as one cached row (it is not a draw and has no rows to slice).
Draws = collections.namedtuple('Draws', 't_rand noise0 u noise1 t_lin')


def _rows(x, i, j):
    """Rows [i, j) of a tensor, of every tensor of an output dict or of a Draws record (None stays None)."""
    if isinstance(x, dict):
        return {k: v[i:j] for k, v in x.items()}
    if isinstance(x, Draws):
        return Draws(*[_rows(t, i, j) for t in x[:4]], x.t_lin)
    return None if x is None else x[i:j]


def _workspace(device, nbytes):
    """Scratch for one render_rays call (raw / z / weights of the two passes), allocated per call on the
    stream that is current: torch's caching allocator recycles the block and keeps its reuse ordered
    on that stream, so renders enqueued on different streams never share scratch."""
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)


_side_streams = {}
_draw_streams = {}


def _draw_stream(device):
    """The stream the whole-batch path makes its random draws on (see Renderer._launch_batch)."""
    s = _draw_streams.get(device)
    if s is None:
        s = torch.cuda.Stream(device=device)
        _draw_streams[device] = s
    return s


def _chunk_streams(device, n=2):
    """The two side streams of the opt-in chunk-overlap mode of render_batch."""
    s = _side_streams.get(device)
    if s is None:
        s = [torch.cuda.Stream(device=device) for _ in range(n)]
        _side_streams[device] = s
    return s


_linspace_cache = {}


def _linspace01(n, device):
    key = (n, device)
    t = _linspace_cache.get(key)
    if t is None:
        t = torch.linspace(0., 1., steps=n, device=device)
        _linspace_cache[key] = t
    return t


def _pytest_uniform(shape, device):
    """np.random.seed(0); np.random.rand(*shape) -> fp32 (render_utils.py:124-127)."""
    np.random.seed(0)
    return torch.Tensor(np.random.rand(*list(shape))).to(device)


class _Raw2OutputsFn(torch.autograd.Function):
    """raw2outputs with a HIP backward (nerf_amd_raw2outputs_backward) with respect to ``raw`` and to
    ``rays_d`` (dists scale with |rays_d|, render_utils.py:259).  z_vals are constants."""

    @staticmethod
    def forward(ctx, raw, z, d, noise, white):
        dev = raw.device
        R, S, ch = raw.shape
        f = dict(device=dev, dtype=torch.float32)
        rgb_map, disp_map, acc_map = torch.empty(R, 3, **f), torch.empty(R, **f), torch.empty(R, **f)
        weights, depth_map = torch.empty(R, S, **f), torch.empty(R, **f)
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_raw2outputs(raw.data_ptr(), ch, z.data_ptr(), d.data_ptr(), d.stride(0), _lib.ptr(noise),
                                                R, S, int(white), rgb_map.data_ptr(), disp_map.data_ptr(),
                                                acc_map.data_ptr(), weights.data_ptr(), depth_map.data_ptr(),
                                                _lib.stream_of(dev)), "nerf_amd_raw2outputs")
        ctx.save_for_backward(raw, z, d, noise if noise is not None else torch.empty(0, device=dev))
        ctx.white = white
        ctx.set_materialize_grads(False)
        return rgb_map, disp_map, acc_map, weights, depth_map

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_w, g_depth):
        raw, z, d, noise = ctx.saved_tensors
        noise = noise if noise.numel() else None
        R, S, ch = raw.shape
        g = [None if t is None else t.contiguous().float() for t in (g_rgb, g_disp, g_acc, g_depth, g_w)]
        g_raw = torch.empty_like(raw)
        g_d = torch.empty(R, 3, device=raw.device, dtype=torch.float32) if ctx.needs_input_grad[2] else None
        with torch.cuda.device(raw.device):
            _lib.check(lib.nerf_amd_raw2outputs_backward(raw.data_ptr(), ch, z.data_ptr(), d.data_ptr(), d.stride(0),
                                                         _lib.ptr(noise), R, S, int(ctx.white), _lib.ptr(g[0]),
                                                         _lib.ptr(g[1]), _lib.ptr(g[2]), _lib.ptr(g[3]), _lib.ptr(g[4]),
                                                         g_raw.data_ptr(), _lib.ptr(g_d), _lib.stream_of(raw.device)),
                       "nerf_amd_raw2outputs_backward")
        return g_raw, None, g_d, None, None


class Renderer(torch.nn.Module):
    def __init__(self, perturb=True, N_importance=128, N_samples=64, use_viewdirs=True,
                 white_bkgd=True, raw_noise_std=0.0, ndc=False, lindisp=False,
                 near=0.0, far=1.0):
        """
        Stores values as class data.
        """
        super(Renderer, self).__init__()
        self.perturb = perturb
        self.N_importance = N_importance
        self.N_samples = N_samples
        self.use_viewdirs = use_viewdirs
        self.white_bkgd = white_bkgd
        self.raw_noise_std = raw_noise_std
        self.ndc = ndc
        self.lindisp = lindisp
        self.near = near
        self.far = far
        if os.environ.get("NERF_AMD_QUIET") != "1":
            print(self.__dict__)     # the reference prints its configuration (render_utils.py:32)

    # ------------------------------------------------------------------ wrappers
    def render_from_pose(self, H, W, K, chunk, c2w, coarse_model, fine_model, retraw=True):
        rgb, disp, acc, extras = self.render(
            H, W, K, coarse_model, fine_model, chunk=chunk, c2w=c2w, retraw=retraw)
        return rgb, disp, acc, extras

    def render_from_rays(self, H, W, K, chunk, rays, coarse_model, fine_model, retraw=True):
        rgb, disp, acc, extras = self.render(H, W, K, coarse_model, fine_model,
                                             chunk=chunk, rays=rays, retraw=retraw)
        return rgb, disp, acc, extras

    def render_path(self):
        pass

    # ------------------------------------------------------------------ core
    def _cfg(self, precision):
        cfg = _lib.RenderCfg()
        cfg.N_samples, cfg.N_importance = int(self.N_samples), int(self.N_importance)
        cfg.perturb = int(self.perturb > 0.)
        cfg.lindisp, cfg.white_bkgd = int(bool(self.lindisp)), int(bool(self.white_bkgd))
        cfg.use_noise = int(self.raw_noise_std > 0.)
        cfg.precision = precision
        return cfg

    @staticmethod
    def _check_model(m, name):
        if not isinstance(m, NeRF):
            raise TypeError("%s must be a nerf_shared_amd.nerf.NeRF or a reference-style NeRF module (got %s)" % (name, type(m).__name__))

    def _handles(self, dev, coarse_model, fine_model):
        """Library handles (re-packed if the weights changed), render cfg and output width."""
        self._check_model(coarse_model, "coarse_model")
        if fine_model is not None:
            self._check_model(fine_model, "fine_model")
        use_fine = fine_model is not None and int(self.N_importance) > 0
        coarse_model._ensure_handle(dev)
        if use_fine:
            fine_model._ensure_handle(dev)
        prec = coarse_model._precision_code()
        if use_fine and fine_model._precision_code() != prec:
            prec = _lib.PREC_FP32
        # only the packed copy this precision reads; a bf16 render also reads the folded stream (feature_linear folded into
        # views_linears.0, include/nerf_amd.h NERF_AMD_COPY_BF16_FOLD), which only the calls that render ask for
        copies = _lib.COPY_OF[prec] | (_lib.COPY_BF16_FOLD if prec == _lib.PREC_BF16 else 0)
        hc = coarse_model._model_handle(dev, copies)
        hf = fine_model._model_handle(dev, copies) if use_fine else None
        return hc, hf, self._cfg(prec), lib.nerf_amd_model_out_ch(hc)

    _UNFILLED = object()          # _draws(into=_UNFILLED): allocate what would be drawn, draw nothing (_draw_buffers)

    def _draws(self, R, dev, pytest=False, into=None):
        """The random draws of one render_rays call on R rays, as a Draws record.  The one place that knows the reference's
        order, shapes and conditions: t_rand [R, Nc] under perturb, noise0 [R, Nc] under raw_noise_std, and with
        N_importance > 0 u [R, Ni] (perturb == 0: nothing is drawn, t_lin is the cached linspace) and noise1 [R, Nc + Ni]
        (render_utils.py:121,264, utils.py:86).  Two ways of producing them:
          into=None     new tensors: torch.rand / torch.randn(...) * raw_noise_std, or with pytest=True the reference's seeded
                        numpy draws (np.random.seed(0); np.random.rand(*shape) each; the deterministic u its broadcast linspace);
          into=a Draws  of row slices [R, .] of the caller's buffers (_draw_buffers, _rows), filled in place: slice.uniform_() /
                        slice.normal_() consume the generator exactly like torch.rand / torch.randn of the same shape.  The
                        noise is left UNSCALED: the caller multiplies each whole buffer once (_scale_noise), not once per chunk."""
        Nc, Ni, std = int(self.N_samples), int(self.N_importance), self.raw_noise_std
        if into is self._UNFILLED:
            uniform = normal = lambda name, shape: torch.empty(shape, device=dev, dtype=torch.float32)
        elif into is not None:
            uniform = lambda name, shape: getattr(into, name).uniform_()
            normal = lambda name, shape: getattr(into, name).normal_()
        elif pytest:
            uniform = lambda name, shape: _pytest_uniform(shape, dev)
            normal = lambda name, shape: _pytest_uniform(shape, dev) * std
        else:
            uniform = lambda name, shape: torch.rand(shape, device=dev)
            normal = lambda name, shape: torch.randn(shape, device=dev) * std
        jitter, noisy = self.perturb > 0., std > 0.
        t_rand = uniform('t_rand', [R, Nc]) if jitter else None
        noise0 = normal('noise0', [R, Nc]) if noisy else None
        u = noise1 = t_lin = None
        if Ni > 0:
            if jitter:
                u = uniform('u', [R, Ni])
            elif pytest:
                np.random.seed(0)
                u = torch.Tensor(np.ascontiguousarray(np.broadcast_to(np.linspace(0., 1., Ni), [R, Ni]))).to(dev)
            else:
                t_lin = _linspace01(Ni, dev)
            noise1 = normal('noise1', [R, Nc + Ni]) if noisy else None
        return Draws(t_rand, noise0, u, noise1, t_lin)

    def _draw_buffers(self, N, dev):
        """Uninitialised buffers for the draws of N rays, for the in-place form of _draws to fill chunk by chunk."""
        return self._draws(N, dev, into=self._UNFILLED)

    def _scale_noise(self, bufs):
        """What the in-place form of _draws leaves to its caller: raw_noise_std times each whole noise buffer, once."""
        for t in (bufs.noise0, bufs.noise1):
            if t is not None:
                t.mul_(self.raw_noise_std)

    def _io(self, rays, draws, outs, z_pre, ws, rows=None):
        """The nerf_amd_render_io of one library call: contiguous fp32 rays [R, 8|11], their Draws record, the dict of output
        tensors, coarse depths [R, N_samples] made in front (or None: the library makes them from t_rand) and the workspace.
        rows=(i, j): the call covers rows [i, j) of all of these (the workspace is the call's own)."""
        if rows is not None:
            rays, draws, outs, z_pre = (_rows(x, *rows) for x in (rays, draws, outs, z_pre))
        io = _lib.RenderIO()
        io.rays, io.ray_ch = rays.data_ptr(), rays.shape[1]
        io.t_vals = _linspace01(int(self.N_samples), rays.device).data_ptr()
        io.t_rand, io.noise0, io.u, io.noise1, io.t_lin_imp = (_lib.ptr(t) for t in draws)
        io.z_coarse = _lib.ptr(z_pre)
        for k in _IO_OUT_KEYS:
            setattr(io, k, _lib.ptr(outs.get(k)))
        io.workspace, io.workspace_bytes = ws.data_ptr(), ws.numel()
        return io

    def _chunk_inputs(self, rays, pytest):
        """What one render_rays call prepares in front of the library: its draws, and with a coarse_sampler its coarse
        depths (else None: the library computes the reference ladder itself)."""
        R, dev = rays.shape[0], rays.device
        draws, z_pre = self._draws(R, dev, pytest), None
        if self.coarse_sampler is not None and R > 0:
            z_pre = torch.empty(R, int(self.N_samples), device=dev, dtype=torch.float32)
            with torch.cuda.device(dev):
                self._coarse_z(rays, draws.t_rand, z_pre)
        return draws, z_pre

    def _launch(self, rays, coarse_model, fine_model, outs, pytest=False):
        """Enqueue render_rays for contiguous fp32 rays [R, 8|11]; writes into the
        tensors of ``outs`` (rows [0, R)).  The draws, depths and scratch it allocates go back to the caching allocator
        on return: their reuse is ordered on the stream that is current, behind the launches that read them."""
        dev = rays.device
        hc, hf, cfg, out_ch = self._handles(dev, coarse_model, fine_model)
        draws, z_pre = self._chunk_inputs(rays, pytest)
        ws = _workspace(dev, lib.nerf_amd_render_rays_workspace(cfg, rays.shape[0], out_ch))
        io = self._io(rays, draws, outs, z_pre, ws)
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_render_rays(cfg, hc, hf, io, rays.shape[0], _lib.stream_of(dev)), "nerf_amd_render_rays")

    # ------------------------------------------------------------------ occupancy grid (opt-in)
    occupancy = None              # a nerf_shared_amd.occupancy.OccupancyGrid: the no-grad render calls evaluate the field at
                                  # its live points only (nerf_amd_render_rays_culled); None: the dense path, untouched
    last_cull = None              # with a grid: the points of the last call, summed over its launches, as host ints
    CULL_GROUP_RAYS = 32768       # rays per culled library call (each call synchronises once per pass)

    def _check_cullable(self, mode):
        """The culled path is forward-only and noise-free; anything else is refused rather than silently rendered densely."""
        if mode != "none":
            raise _lib.NerfAmdError("Renderer.occupancy is set and this call asks for gradients: the occupancy grid culls in the "
                                    "no-grad render path only.  Render under torch.no_grad() (or with frozen models and rays), or "
                                    "set renderer.occupancy = None for training and pose estimation")
        if self.raw_noise_std > 0.:
            raise _lib.NerfAmdError("Renderer.occupancy is set and raw_noise_std > 0: sigma noise would resurrect culled samples.  "
                                    "Set raw_noise_std = 0 (as every evaluation render does) or renderer.occupancy = None")

    def _launch_culled(self, rays, coarse_model, fine_model, outs, pytest, stats):
        """render_rays of one chunk's rays [R, 8|11] through nerf_amd_render_rays_culled into the rows of ``outs``: the
        chunk's draws (and sampler depths) are made once, as _launch makes them, and the library is called per group of at
        most CULL_GROUP_RAYS rays on the matching rows.  Adds the four counts to ``stats``."""
        dev, grid = rays.device, self.occupancy
        if grid.device != dev:
            raise _lib.NerfAmdError("Renderer.occupancy is on %s, the rays on %s" % (grid.device, dev))
        hc, hf, cfg, out_ch = self._handles(dev, coarse_model, fine_model)
        R, step = rays.shape[0], self.CULL_GROUP_RAYS
        draws, z_pre = self._chunk_inputs(rays, pytest)
        g = grid._c()
        counts = (ctypes.c_int64 * 4)()
        ws = _workspace(dev, lib.nerf_amd_render_rays_culled_workspace(cfg, min(R, step), out_ch))
        for i in range(0, R, step):
            j = min(i + step, R)
            io = self._io(rays, draws, outs, z_pre, ws, rows=(i, j))
            with torch.cuda.device(dev):
                _lib.check(lib.nerf_amd_render_rays_culled(cfg, hc, hf, io, j - i, ctypes.byref(g), counts, _lib.stream_of(dev)),
                           "nerf_amd_render_rays_culled")
            for n, k in enumerate(stats):
                stats[k] += int(counts[n])


    @staticmethod
    def _new_cull_stats():          # in the order of nerf_amd_render_rays_culled's four counts
        return {'coarse_live': 0, 'coarse_total': 0, 'fine_live': 0, 'fine_total': 0}

    # ------------------------------------------------------------------ occupancy grid in training and pose estimation (opt-in)
    train_occupancy = None        # a nerf_shared_amd.occupancy.TrainCull: a call in "train" mode (parameters or rays ask for
                                  # gradients, the training kernels cover the models) evaluates each field at a compact list
                                  # of fixed capacity; nothing synchronises, so a captured step captures it.  None: the dense
                                  # training path, launch for launch.  A no-grad call ignores it (that is `occupancy`).

    def _field_culled(self, cull, net, rays, z, fine_pass):
        """raw [R, S, ch] of one pass with the field evaluated at the kept points only: capped cull -> the training kernels in
        their explicit-points mode on the compact list (R = C, S = 1; a model that asks for no gradient keeps its forward-only
        kernel, nerf_amd_field_points, on the same list) -> expand.  Culled and overflowing samples have raw = +0.0."""
        from . import occupancy as occ
        R, S = z.shape
        dev = rays.device
        if net.use_viewdirs and rays.shape[1] != 11:
            raise _lib.NerfAmdError("a model with a view branch needs rays [N, 11], got %s" % (tuple(rays.shape),))
        pts, vd, rank, src = cull.cull(rays, z, fine_pass)
        if not net.use_viewdirs:
            vd = None
        C = pts.shape[0]
        if net._grad_request(dev, rays)[0] == "train":
            raw_live = nerf_mod._train_field(net, net._train_precision(), pts, vd, None, None, C, 1)
        else:
            with torch.no_grad():
                handle = net._model_handle(dev)
                raw_live = torch.empty(C, 4 if net.use_viewdirs else net.output_ch, device=dev, dtype=torch.float32)
                with torch.cuda.device(dev):
                    _lib.check(lib.nerf_amd_field_points(handle, pts.data_ptr(), _lib.ptr(vd), C, raw_live.data_ptr(),
                                                         net._precision_code(), _lib.stream_of(dev)), "nerf_amd_field_points")
        return occ._ExpandFn.apply(raw_live, rank, src).reshape(R, S, raw_live.shape[1])

    # ------------------------------------------------------------------ ray bounds (opt-in)
    ray_bounds = None             # a nerf_shared_amd.occupancy.RayBounds: render_rays and render_batch (and so every entry
                                  # built on them) first clip each ray's near / far to the span over which its grid is live --
                                  # once per call, on the batch as a whole, before the chunk loop and before any draw.  None:
                                  # the batch goes on as it came, launch for launch.

    def _clip(self, ray_batch):
        """The batch a public entry goes on with: clipped by ray_bounds when one is set."""
        rb = self.ray_bounds
        if rb is None or ray_batch.dim() != 2 or ray_batch.shape[0] == 0:
            return ray_batch
        _lib.require_device(ray_batch, "ray_batch")
        return rb.apply(ray_batch)

    # ------------------------------------------------------------------ coarse sampler (opt-in)
    coarse_sampler = None         # a nerf_shared_amd.occupancy.LiveSampler: every render path takes its coarse depths from it --
                                  # the same stratified ladder and draws, mapped through each ray's live probes -- instead of
                                  # nerf_amd_coarse_z.  None: the reference ladder, launch for launch.

    def _check_sampler(self, dev):
        """What a set coarse_sampler cannot do is refused before any draw or launch."""
        cs = self.coarse_sampler
        if cs is None:
            return
        if self.lindisp:
            raise _lib.NerfAmdError("Renderer.coarse_sampler is set and lindisp is on: the live-stretch warp is defined in depth, not "
                                    "in disparity.  Set lindisp = False or renderer.coarse_sampler = None")
        if cs.grid.device != dev:
            raise _lib.NerfAmdError("Renderer.coarse_sampler is on %s, the rays on %s" % (cs.grid.device, dev))

    def _coarse_z(self, rays, t_rand, z_out):
        """The coarse depths of contiguous fp32 rays [R, 8|11] into z_out [R, N_samples], on the current stream: nerf_amd_coarse_z,
        or the coarse_sampler's kernel when one is set.  t_rand [R, N_samples] | None: the jitter draws (read under perturb).
        Called with the rays' device current (inside torch.cuda.device(dev)), like the library calls around it."""
        dev, Nc = rays.device, int(self.N_samples)
        cs = self.coarse_sampler
        if cs is not None:
            self._check_sampler(dev)
            cs.fill(rays, _linspace01(Nc, dev), t_rand if self.perturb > 0. else None, z_out)
            return
        _lib.check(lib.nerf_amd_coarse_z(rays.data_ptr(), rays.shape[1], _linspace01(Nc, dev).data_ptr(), _lib.ptr(t_rand),
                                         rays.shape[0], Nc, int(bool(self.lindisp)), int(self.perturb > 0.), z_out.data_ptr(),
                                         _lib.stream_of(dev)), "nerf_amd_coarse_z")

    def _draw_chunks(self, N, dev, spans):
        """The draws of every chunk of a batch in whole-batch buffers: the reference's order inside every render_rays call
        (t_rand, noise0, u, noise1 of chunk 0, then of chunk 1, ...), each into its rows of one buffer per kind, so the
        result equals per-chunk render_rays calls bit for bit."""
        bufs = self._draw_buffers(N, dev)
        for i, j in spans:
            self._draws(j - i, dev, into=_rows(bufs, i, j))
        self._scale_noise(bufs)
        return bufs

    def _launch_batch(self, rays, spans, coarse_model, fine_model, full):
        """render_batch as ONE library call over whole-batch buffers (nerf_amd_render_batch), draws per chunk (_draw_chunks):
        the library is free to launch in groups that suit the GPU and to run the per-ray kernels beside the field kernels."""
        dev, N = rays.device, rays.shape[0]
        hc, hf, cfg, out_ch = self._handles(dev, coarse_model, fine_model)
        z_all = torch.empty(N, int(self.N_samples), device=dev, dtype=torch.float32)
        if self.perturb > 0. or self.raw_noise_std > 0.:
            # The draws depend on nothing but the generator (whose state lives on the host), so they go on a stream of
            # their own: the dozens of small RNG launches of this call then run beside whatever the device is still busy
            # with (the field kernels of the previous frame, when frames are rendered back to back) instead of in front
            # of this frame's first field kernel.  Same values as on the caller's stream.
            cur, ds = torch.cuda.current_stream(dev), _draw_stream(dev)
            with torch.cuda.stream(ds):
                bufs = self._draw_chunks(N, dev, spans)
                drawn = torch.cuda.Event()
                drawn.record(ds)
            cur.wait_event(drawn)
            for t in bufs[:4]:                                 # allocated on the draw stream, consumed on the caller's
                if t is not None:
                    t.record_stream(cur)
        else:
            bufs = self._draws(N, dev)                         # nothing to draw: the deterministic u, if any
        ws = _workspace(dev, lib.nerf_amd_render_batch_workspace(cfg, N, out_ch))
        io = self._io(rays, bufs, full, z_all, ws)
        with torch.cuda.device(dev):
            self._coarse_z(rays, bufs.t_rand, z_all)
            # the library's side stream reads the buffers too; its work is ordered before the caller's stream continues, so
            # releasing them to the caching allocator (stream-ordered on the caller's stream) on return is safe
            _lib.check(lib.nerf_amd_render_batch(cfg, hc, hf, io, N, _lib.stream_of(dev)), "nerf_amd_render_batch")

    def _launch_chunks(self, rays, spans, coarse_model, fine_model, full):
        """render_batch's chunk loop as one library call (nerf_amd_render_chunks): per-chunk draws (_draw_chunks) and
        output rows exactly as _launch makes them, two workspaces used alternately, and the coarse depths of all chunks
        from one launch in front."""
        dev, N, n = rays.device, rays.shape[0], len(spans)
        hc, hf, cfg, out_ch = self._handles(dev, coarse_model, fine_model)
        z_all = torch.empty(N, int(self.N_samples), device=dev, dtype=torch.float32)
        bufs = self._draw_chunks(N, dev, spans)
        nbytes = lib.nerf_amd_render_rays_workspace(cfg, max(j - i for i, j in spans), out_ch)
        wss = [_workspace(dev, nbytes), _workspace(dev, nbytes)]
        ios = (_lib.RenderIO * n)(*[self._io(rays, bufs, full, z_all, wss[k % 2], rows=s) for k, s in enumerate(spans)])
        counts = (ctypes.c_int64 * n)(*[j - i for i, j in spans])
        with torch.cuda.device(dev):
            self._coarse_z(rays, bufs.t_rand, z_all)
            _lib.check(lib.nerf_amd_render_chunks(cfg, hc, hf, ios, counts, n, _lib.stream_of(dev)), "nerf_amd_render_chunks")

    def _launch_overlapped(self, rays, spans, coarse_model, fine_model, full):
        """render_batch's chunk loop with consecutive chunks alternating between two side streams (overlap_chunks)."""
        dev = rays.device
        # pack parameters and build the cached linspaces on the caller's stream first, then fan out
        _linspace01(int(self.N_samples), dev)
        if self.N_importance > 0:
            _linspace01(int(self.N_importance), dev)
        self._handles(dev, coarse_model, fine_model)
        cur = torch.cuda.current_stream(dev)
        ready = torch.cuda.Event()
        ready.record(cur)
        side = _chunk_streams(dev)
        for s in side:
            s.wait_event(ready)
        for n, (i, j) in enumerate(spans):
            with torch.cuda.stream(side[n % len(side)]):      # draws and scratch are made on the chunk's own stream
                self._launch(rays[i:j], coarse_model, fine_model, _rows(full, i, j))
        for s in side:
            cur.wait_stream(s)
        for v in full.values():
            v.record_stream(side[0]); v.record_stream(side[1])

    def _render_rays_train(self, rays, coarse_model, fine_model, retraw, retweights, pytest):
        """render_rays with autograd into the models' parameters (what main.py:77-104 needs):
        the same kernels stage by stage -- z_vals, training forward of the field (activations
        saved), compositing -- with the field and raw2outputs as autograd Functions whose
        backward passes are HIP kernels.  z_samples are detached, as in the reference
        (render_utils.py:145); `rays` may require grad (pose estimation)."""
        R, dev = rays.shape[0], rays.device
        Nc, Ni = int(self.N_samples), int(self.N_importance)
        t_rand, noise0, u, noise1, t_lin = self._draws(R, dev, pytest)
        f = dict(device=dev, dtype=torch.float32)
        stream = _lib.stream_of(dev)
        z = torch.empty(R, Nc, **f)
        with torch.cuda.device(dev):
            self._coarse_z(rays, t_rand, z)
        rays_d = rays[:, 3:6]            # a view: composite gradients with respect to |d| flow back into `rays`

        cull = self.train_occupancy
        if cull is not None and self.raw_noise_std > 0.:
            raise _lib.NerfAmdError("Renderer.train_occupancy is set and raw_noise_std > 0: sigma noise would resurrect culled samples.  "
                                    "Set raw_noise_std = 0 or renderer.train_occupancy = None")

        def field(net, zz):
            # a model that asks for no gradient (frozen, and the rays carry none) keeps its own forward-only kernel and
            # precision; only models that train go through the training kernels
            if cull is not None:
                return self._field_culled(cull, net, rays, zz, zz is not z_c)
            if net._grad_request(dev, rays)[0] == "train":
                return net.forward_rays(rays, zz)
            with torch.no_grad():
                pts = rays[:, None, 0:3] + rays[:, None, 3:6] * zz[:, :, None]      # render_utils.py:131, two rounded ops
                return net.forward(pts, rays[:, 8:11] if rays.shape[1] > 8 else None)

        z_c = z

        raw = field(coarse_model, z)
        rgb, disp, acc, weights, _ = _Raw2OutputsFn.apply(raw, z, rays_d, noise0, bool(self.white_bkgd))
        ret = {}
        if Ni > 0:
            rgb0, disp0, acc0 = rgb, disp, acc
            z_f, z_std = torch.empty(R, Nc + Ni, **f), torch.empty(R, **f)
            w_c = weights.detach()
            with torch.cuda.device(dev):
                _lib.check(lib.nerf_amd_resample(z.data_ptr(), w_c.data_ptr(), _lib.ptr(u), _lib.ptr(t_lin), R, Nc, Ni,
                                                 z_f.data_ptr(), z_std.data_ptr(), stream), "nerf_amd_resample")
            z = z_f
            net = coarse_model if fine_model is None else fine_model
            raw = field(net, z)
            rgb, disp, acc, weights, _ = _Raw2OutputsFn.apply(raw, z, rays_d, noise1, bool(self.white_bkgd))
        ret.update(rgb_map=rgb, disp_map=disp, acc_map=acc)
        if retraw:
            ret['raw'] = raw
        if retweights:
            ret['weights'] = weights
            ret['z_vals'] = z
        if Ni > 0:
            ret.update(rgb0=rgb0, disp0=disp0, acc0=acc0, z_std=z_std)
        return ret

    def _alloc_outputs(self, R, dev, out_ch, retraw, retweights):
        Ni = int(self.N_importance)
        S_last = int(self.N_samples) + Ni
        f = dict(device=dev, dtype=torch.float32)
        outs = {'rgb_map': torch.empty(R, 3, **f), 'disp_map': torch.empty(R, **f), 'acc_map': torch.empty(R, **f)}
        if retraw:
            outs['raw'] = torch.empty(R, S_last, out_ch, **f)
        if retweights:
            outs['weights'] = torch.empty(R, S_last, **f)
            outs['z_vals'] = torch.empty(R, S_last, **f)
        if Ni > 0:
            outs['rgb0'] = torch.empty(R, 3, **f)
            outs['disp0'] = torch.empty(R, **f)
            outs['acc0'] = torch.empty(R, **f)
            outs['z_std'] = torch.empty(R, **f)
        return outs

    def _grad_mode(self, coarse_model, fine_model, rays):
        """The models' gradient requests for one call, combined: "train" only if every model that asks for gradients is
        covered by the training kernels; one uncovered model defers the whole call (nerf.NeRF._grad_request)."""
        reqs = [coarse_model._grad_request(rays.device, rays)]
        if fine_model is not None and self.N_importance > 0:
            reqs.append(fine_model._grad_request(rays.device, rays))
        for m, d in reqs:
            if m == "defer":
                return m, d
        return ("train", None) if any(m == "train" for m, _ in reqs) else ("none", None)

    def render_rays(self, ray_batch, coarse_model, fine_model, retraw=False, retweights=False,
                    verbose=False, pytest=False):
        """Volumetric rendering of one ray batch (render_utils.py:67-174).

        ray_batch [N, 8|11] = origin, direction, near, far, (unit view dir).
        Returns the reference's dict: rgb_map, disp_map, acc_map, [raw],
        [weights, z_vals], and with N_importance > 0: rgb0, disp0, acc0, z_std.
        """
        ret = self._render("ray_batch", self._clip(ray_batch), coarse_model, fine_model, None, retraw, retweights, pytest)
        if DEBUG:
            for k in ret:
                if torch.isnan(ret[k]).any() or torch.isinf(ret[k]).any():
                    print(f"! [Numerical Error] {k} contains nan or inf.")
        return ret

    pipeline_batch = True         # render_batch: one library call over whole-batch buffers (nerf_amd_render_batch): launch
                                  # groups of 32768 rays, per-ray kernels on a side stream beside the next field kernel
    fuse_chunk_launches = True    # (pipeline_batch off) one library call per chunk list (three dependent launches per chunk)
    overlap_chunks = False        # (pipeline_batch off) opt-in: two-stream chunk pipeline, two field kernels at a time

    def render_batch(self, coarse_model, fine_model, rays_flat, chunk=1024 * 32, retraw=False):
        """Render rays in chunks (render_utils.py:51-65).  Outputs of every chunk land
        directly in one preallocated tensor per key (the reference's per-key torch.cat,
        without the copy).  By default (``Renderer.pipeline_batch``) the whole batch goes to the
        library in one call: `chunk` then only decides how the random draws are grouped (as in
        the reference), not how the GPU is launched -- every kernel is per-ray independent, so the
        result is the same bit for bit.  The older modes remain for A/B runs:
        with ``Renderer.overlap_chunks = True`` consecutive chunks
        alternate between two HIP streams (each with its own workspace) so the small
        per-ray kernels and launch/drain gaps of one chunk hide under the field kernel
        of the other; results do not depend on it (random draws come from the device's one
        generator in chunk order in every mode).  Off by default: the gain is ~3 % and
        concurrent kernels blur per-kernel timings."""
        return self._render("rays_flat", self._clip(rays_flat), coarse_model, fine_model, chunk, retraw)

    def _render(self, name, ray_batch, coarse_model, fine_model, chunk, retraw, retweights=False, pytest=False):
        """render_rays and render_batch behind the ray-bounds clip: one preamble and one statement of the choice between
        the culled, the training and the dense path (a deferred gradient: the dense path, with a backward that explains
        itself, nerf._grad_request).  Every path works chunk by chunk, a chunk being one render_rays call of the
        reference with its own draws.  chunk=None is render_rays: the batch, empty or not, is the one chunk; it is passed on
        unsliced and always goes to the library as one nerf_amd_render_rays call."""
        _lib.require_device(ray_batch, name)
        coarse_model, fine_model = nerf_mod.adopt(coarse_model), nerf_mod.adopt(fine_model)     # reference-class models: a twin sharing their parameters
        rays = ray_batch.detach().contiguous().float()
        if rays.dim() != 2 or rays.shape[1] not in (8, 11):
            raise _lib.NerfAmdError("%s must be [N, 8] or [N, 11], got %s" % (name, tuple(ray_batch.shape)))
        self._check_model(coarse_model, "coarse_model")
        if fine_model is not None:
            self._check_model(fine_model, "fine_model")
        N, dev = rays.shape[0], rays.device
        self._check_sampler(dev)
        mode, deferred = self._grad_mode(coarse_model, fine_model, ray_batch) if N > 0 else ("none", None)
        out_ch = 4 if coarse_model.use_viewdirs else coarse_model.output_ch
        spans = [(0, N)] if chunk is None else [(i, min(i + chunk, N)) for i in range(0, N, chunk)]
        if self.occupancy is not None:     # per chunk (the reference's draws), the library called per group of <= 32768 rays
            self._check_cullable(mode)
            ret = self._alloc_outputs(N, dev, out_ch, retraw, retweights)
            stats = self._new_cull_stats()
            for i, j in spans:
                self._launch_culled(rays[i:j], coarse_model, fine_model, _rows(ret, i, j), pytest, stats)
            self.last_cull = stats
        elif mode == "train":              # an autograd graph per chunk, concatenated like the reference
            live = ray_batch if (torch.is_grad_enabled() and ray_batch.requires_grad) else rays
            parts = [self._render_rays_train((live if chunk is None else live[i:j]).contiguous().float(), coarse_model,
                                             fine_model, retraw, retweights, pytest) for i, j in spans]
            # (one chunk: the tensors themselves -- the reference's torch.cat of a single tensor is a copy of it)
            ret = parts[0] if len(parts) == 1 else {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}
        else:
            ret = self._alloc_outputs(N, dev, out_ch, retraw, retweights)
            if chunk is not None and self.pipeline_batch and N > 0 and (len(spans) > 1 or N > 49152):
                self._launch_batch(rays, spans, coarse_model, fine_model, ret)
            elif len(spans) > 1 and self.overlap_chunks:
                self._launch_overlapped(rays, spans, coarse_model, fine_model, ret)
            elif len(spans) > 1 and self.fuse_chunk_launches:
                self._launch_chunks(rays, spans, coarse_model, fine_model, ret)
            else:
                for i, j in spans:
                    self._launch(rays[i:j], coarse_model, fine_model, _rows(ret, i, j), pytest)
        if retweights and ret['weights'].shape[1] == 1:
            ret['weights'] = ret['weights'][:, :0]                             # one sample: see raw2outputs
        return nerf_mod.attach_deferred_grad(ret, deferred)

    def render(self, H, W, K, coarse_model, fine_model, chunk=1024 * 32, rays=None, retraw=True,
               c2w=None, c2w_staticcam=None):
        """Render a full image from ``c2w`` or an explicit ray set (render_utils.py:176-238).
        Returns [rgb_map, disp_map, acc_map, extras]."""
        coarse_model, fine_model = nerf_mod.adopt(coarse_model), nerf_mod.adopt(fine_model)
        if c2w is not None:
            dev = next(coarse_model.parameters()).device
            if not dev.type == 'cuda':
                raise _lib.NerfAmdError("models are on %s; nerf_shared_amd runs on ROCm devices only" % dev)
            batch = utils.make_ray_batch(H, W, K, c2w, self.near, self.far, self.use_viewdirs, self.ndc,
                                         c2w_staticcam=c2w_staticcam, device=dev)
            sh = (H, W, 3)
        else:
            rays_o, rays_d = rays
            _lib.require_device(rays_d, "rays")
            sh = rays_d.shape
            tracked = torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad)
            if (not tracked and c2w_staticcam is None and rays_o.dtype == torch.float32 and rays_d.dtype == torch.float32
                    and rays_o.is_cuda and rays_o.shape == rays_d.shape and rays_d.numel() > 0):
                # no gradient flows into the rays: the ten small launches below as one (nerf_amd_assemble_rays)
                src = rays_d.detach().reshape(-1, 3).contiguous() if self.use_viewdirs else None
                o, d = rays_o.detach(), rays_d.detach()
                if self.ndc:
                    o, d = utils.ndc_rays(H, W, K[0][0], 1., o, d)
                o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
                batch = torch.empty(o.shape[0], 11 if self.use_viewdirs else 8, device=o.device, dtype=torch.float32)
                with torch.cuda.device(o.device):
                    _lib.check(lib.nerf_amd_assemble_rays(o.data_ptr(), d.data_ptr(), _lib.ptr(src), o.shape[0], float(self.near),
                                                          float(self.far), batch.data_ptr(), _lib.stream_of(o.device)),
                               "nerf_amd_assemble_rays")
            else:
                viewdirs = None
                if self.use_viewdirs:
                    viewdirs = rays_d
                    if c2w_staticcam is not None:
                        rays_o, rays_d = utils.get_rays(H, W, K, c2w_staticcam)
                    viewdirs = viewdirs / torch.norm(viewdirs, dim=-1, keepdim=True)
                    viewdirs = torch.reshape(viewdirs, [-1, 3]).float()
                sh = rays_d.shape
                if self.ndc:
                    rays_o, rays_d = utils.ndc_rays(H, W, K[0][0], 1., rays_o, rays_d)
                rays_o = torch.reshape(rays_o, [-1, 3]).float()
                rays_d = torch.reshape(rays_d, [-1, 3]).float()
                near, far = self.near * torch.ones_like(rays_d[..., :1]), self.far * torch.ones_like(rays_d[..., :1])
                batch = torch.cat([rays_o, rays_d, near, far], -1)
                if self.use_viewdirs:
                    batch = torch.cat([batch, viewdirs], -1)

        all_ret = self.render_batch(coarse_model, fine_model, batch, chunk, retraw)
        for k in all_ret:
            k_sh = list(sh[:-1]) + list(all_ret[k].shape[1:])
            all_ret[k] = torch.reshape(all_ret[k], k_sh)

        ret_list = [all_ret[k] for k in _KEYS_MAIN]
        ret_dict = {k: all_ret[k] for k in all_ret if k not in _KEYS_MAIN}
        return ret_list + [ret_dict]

    def raw2outputs(self, raw, z_vals, rays_d, pytest=False):
        """raw [R,S,>=4], z_vals [R,S], rays_d [R,3] -> rgb_map, disp_map, acc_map,
        weights, depth_map (render_utils.py:241-290).  Differentiable with respect to
        ``raw`` and ``rays_d`` (HIP backward kernel: the intervals scale with |rays_d|);
        z_vals are constants."""
        _lib.require_device(raw, "raw")
        dev = raw.device
        raw_c = raw.detach().contiguous().float()
        if raw_c.dim() != 3 or raw_c.shape[-1] < 4:
            raise _lib.NerfAmdError("raw must be [num_rays, num_samples, >=4]")
        R, S, ch = raw_c.shape
        z = z_vals.detach().contiguous().float()
        d = rays_d.detach().contiguous().float()
        noise = None
        if self.raw_noise_std > 0.:
            noise = (_pytest_uniform([R, S], dev) if pytest else torch.randn([R, S], device=dev)) * self.raw_noise_std
        if torch.is_grad_enabled() and (raw.requires_grad or rays_d.requires_grad):
            out = _Raw2OutputsFn.apply(raw.contiguous().float(), z, rays_d.contiguous().float(), noise, bool(self.white_bkgd))
        else:
            with torch.no_grad():
                out = _Raw2OutputsFn.apply(raw_c, z, d, noise, bool(self.white_bkgd))
        if S == 1:
            # With one sample the reference's `dists` is empty (it expands the 1e10 tail to dists[..., :1].shape = [R, 0],
            # render_utils.py:256-258), and so are alpha and the weights: the kernels return the sums over nothing
            # (background colour, acc 0, disp NaN, zero gradients) and the weights come back as [R, 0].
            out = (out[0], out[1], out[2], out[3][:, :0], out[4])
        return out

    def render_from_batch_poses(self, H, W, K, chunk, batch_c2w, coarse_model, fine_model,
                                retraw, save_directory, b_combine_as_video=False, tb_writer=None, io_workers=4):
        """Render a set of poses and save them as 000.png, 001.png, ... (render_utils.py:293-319).

        The reference copies every float image to the host, quantises it with numpy and writes the
        PNG before it renders the next pose.  Here the image is quantised on the GPU (utils.to8b ->
        nerf_amd_to8b), one quarter of the bytes crosses PCIe into pinned memory on a copy stream,
        and PNG encoding + file writes run on `io_workers` threads while the next pose renders
        (io_workers=0: write synchronously).  Returns the uint8 frames [H, W, 3] (the reference
        returns nothing).  Video output needs imageio's ffmpeg plugin and is skipped without it."""
        from . import image_io
        os.makedirs(save_directory, exist_ok=True)
        keep_float = b_combine_as_video or tb_writer is not None
        rgbs, frames = [], []
        writer = image_io.AsyncImageWriter(io_workers) if io_workers > 0 else None
        copy_stream = None
        try:
            with torch.no_grad():
                for i, c2w in enumerate(batch_c2w):
                    rgb, _, _, _ = self.render_from_pose(H, W, K, chunk=chunk, c2w=c2w,
                                                         coarse_model=coarse_model, fine_model=fine_model)
                    rgb8 = utils.to8b(rgb)
                    filename = os.path.join(save_directory, '{:03d}.png'.format(i))
                    if keep_float:
                        rgbs.append(rgb.cpu().numpy())
                    if writer is None:
                        frames.append(rgb8.cpu().numpy())
                        image_io.write_png(filename, frames[-1])
                        continue
                    dev = rgb8.device
                    if copy_stream is None:
                        copy_stream = torch.cuda.Stream(dev)
                    host = torch.empty(rgb8.shape, dtype=torch.uint8, pin_memory=True)
                    copy_stream.wait_stream(torch.cuda.current_stream(dev))
                    with torch.cuda.stream(copy_stream):
                        host.copy_(rgb8, non_blocking=True)
                        done = torch.cuda.Event()
                        done.record(copy_stream)
                    rgb8.record_stream(copy_stream)
                    frames.append(host.numpy())
                    writer.submit(filename, frames[-1], before=done.synchronize)
        finally:
            if writer is not None:
                writer.close()
        if b_combine_as_video:
            try:
                import imageio
                imageio.mimwrite(os.path.join(save_directory, 'video.mp4'), utils.to8b(np.stack(rgbs)), fps=30, quality=8)
            except ImportError:
                try:                         # no imageio/ffmpeg here: an animated GIF from the uint8 frames instead
                    from PIL import Image
                    imgs = [Image.fromarray(f) for f in frames]
                    imgs[0].save(os.path.join(save_directory, 'video.gif'), save_all=True, append_images=imgs[1:],
                                 duration=33, loop=0)
                    print("render_from_batch_poses: imageio is not installed, wrote video.gif instead of video.mp4")
                except ImportError:
                    print("render_from_batch_poses: neither imageio nor Pillow is installed, video skipped (frames are on disk)")
        if tb_writer is not None:
            tb_writer.add_images('Test/Images', torch.tensor(utils.to8b(np.stack(rgbs))), dataformats="NHWC")
        return frames
