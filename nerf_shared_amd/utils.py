"""Drop-in for the hot-path half of nerf_shared/utils.py: ray generation, the NDC
warp, hierarchical sampling, metrics and the two factories that build models
and renderers from an argparse namespace.

Reference: /root/reference/nerf_shared/utils.py:24-161 for the hot path.  From the
callers either side of it this module also carries the optimizer
factory and checkpoint format (utils.py:163-214, :444-456) and a device-resident version
of the training ray batching (utils.py:360-442).  Dataset loaders are not reproduced
(no datasets offline).
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import lib

# ---------------------------------------------------------------- metrics (utils.py:24-30)
class _Img2MseFn(torch.autograd.Function):
    """mean((x - y)^2) of two fp32 device tensors of one shape: one launch forward, one backward (the torch expression
    is three forward and five backward launches; the loss of main.py:93-98 evaluates it twice per step)."""

    @staticmethod
    def forward(ctx, x, y):
        dev, n = x.device, x.numel()
        out = torch.empty((), device=dev, dtype=torch.float32)
        partials = torch.empty(256, device=dev, dtype=torch.float32) if n > 16384 else None
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_img2mse(x.data_ptr(), y.data_ptr(), n, out.data_ptr(), _lib.ptr(partials),
                                            _lib.stream_of(dev)), "nerf_amd_img2mse")
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        dev = x.device
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        g = g.contiguous().float()
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_img2mse_backward(x.data_ptr(), y.data_ptr(), x.numel(), g.data_ptr(), _lib.ptr(gx),
                                                     _lib.ptr(gy), _lib.stream_of(dev)), "nerf_amd_img2mse_backward")
        return gx, gy


def img2mse(x, y):
    """torch.mean((x - y) ** 2) (utils.py:24).  Two fp32 tensors of one shape on a ROCm device go through the library
    (one launch each way); anything else -- host tensors, broadcasting, other dtypes -- is the reference's expression."""
    if (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.is_cuda and y.is_cuda and x.device == y.device
            and x.dtype == torch.float32 and y.dtype == torch.float32 and x.shape == y.shape and x.numel() > 0
            and x.is_contiguous() and y.is_contiguous()):
        return _Img2MseFn.apply(x, y)
    return torch.mean((x - y) ** 2)


class _Img2MseEachFn(torch.autograd.Function):
    """out[b] = mean((x[b] - y_b)^2) (nerf_amd_img2mse_each): one block per hypothesis, one launch each way; y is a constant."""

    @staticmethod
    def forward(ctx, x, y):
        dev, B = x.device, x.shape[0]
        m = x.numel() // B
        out = torch.empty(B, device=dev, dtype=torch.float32)
        ctx.y_stride = m if y.dim() == x.dim() else 0
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_img2mse_each(x.data_ptr(), y.data_ptr(), ctx.y_stride, m, B, out.data_ptr(), _lib.stream_of(dev)),
                       "nerf_amd_img2mse_each")
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        dev, B = x.device, x.shape[0]
        gx = torch.empty_like(x)
        g = g.contiguous().float()
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_img2mse_each_backward(x.data_ptr(), y.data_ptr(), ctx.y_stride, x.numel() // B, B, g.data_ptr(),
                                                          gx.data_ptr(), _lib.stream_of(dev)), "nerf_amd_img2mse_each_backward")
        return gx, None


POSE_BATCH_MAX, IMG2MSE_EACH_MAX = 1024, 16384          # csrc/kernels.h: hypotheses per launch, values per one-block loss


def img2mse_each(x, y):
    """One img2mse per hypothesis: x [B, ...], y of the same shape or of the shape of one x[b] (shared by all) -> [B], each
    entry bit-equal to img2mse(x[b], y_b).  fp32 contiguous tensors on one ROCm device with B <= 1024 and at most 16384
    values per hypothesis go through the library (one block per hypothesis, one launch each way; y is a constant there);
    anything else is ((x - y) ** 2).flatten(1).mean(1)."""
    if (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.is_cuda and y.is_cuda and x.device == y.device
            and x.dtype == torch.float32 and y.dtype == torch.float32 and x.dim() >= 2 and 1 <= x.shape[0] <= POSE_BATCH_MAX
            and (y.shape == x.shape or y.shape == x.shape[1:]) and 1 <= x[0].numel() <= IMG2MSE_EACH_MAX
            and x.is_contiguous() and y.is_contiguous() and not (y.requires_grad and torch.is_grad_enabled())):
        return _Img2MseEachFn.apply(x, y)
    return ((x - y) ** 2).flatten(1).mean(1)


mse2psnr = lambda x: -10. * torch.log(x) / torch.log(torch.Tensor([10.]).to(x.device))  # noqa: E731


def to8b(x):
    """uint8(255 * clip(x, 0, 1)) (utils.py:30).  numpy in -> numpy out exactly like the reference;
    a device tensor is quantised on the GPU (uint8 device tensor out, one quarter of the bytes to
    copy or gather afterwards)."""
    if isinstance(x, torch.Tensor):
        _lib.require_device(x, "x")
        src = x.detach().contiguous().float()
        if src.data_ptr() % 16:
            src = src.clone()                      # a view into the middle of a storage: the kernel loads 16 bytes at a time
        out = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
        with torch.cuda.device(src.device):
            _lib.check(lib.nerf_amd_to8b(src.data_ptr(), src.numel(), out.data_ptr(), _lib.stream_of(src.device)),
                       "nerf_amd_to8b")
        return out
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def _default_device():
    if not torch.cuda.is_available():
        raise _lib.NerfAmdError("no ROCm device visible; nerf_shared_amd has no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def _host_pose(c2w):
    """First three rows of a camera-to-world matrix as 12 host floats (3x4 row-major)."""
    if isinstance(c2w, torch.Tensor):
        c2w = c2w.detach().cpu().numpy()
    c2w = np.asarray(c2w, dtype=np.float32)
    if c2w.ndim != 2 or c2w.shape[0] < 3 or c2w.shape[1] != 4:
        raise ValueError("c2w must be [>=3, 4], got %s" % (c2w.shape,))
    return np.ascontiguousarray(c2w[:3, :4])


def make_ray_batch(H, W, K, c2w, near, far, use_viewdirs, ndc, c2w_staticcam=None, device=None,
                   pix0=0, n=None):
    """get_rays + viewdirs + (ndc_rays) + near/far assembled as the [n, 8|11] batch
    that Renderer.render builds (render_utils.py:200-226), in one kernel, for the
    flat pixel range [pix0, pix0+n) (default: the whole image)."""
    device = device or _default_device()
    n = H * W - pix0 if n is None else n
    K4 = (ctypes.c_double * 4)(float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
    pose = _host_pose(c2w)
    pose_s = _host_pose(c2w_staticcam) if c2w_staticcam is not None else None
    ch = 11 if use_viewdirs else 8
    out = torch.empty(n, ch, device=device, dtype=torch.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    with torch.cuda.device(device):
        _lib.check(lib.nerf_amd_make_rays(int(H), int(W), K4, pose.ctypes.data_as(fp),
                                          pose_s.ctypes.data_as(fp) if pose_s is not None else None,
                                          int(pix0), int(n), float(near), float(far), int(bool(use_viewdirs)),
                                          int(bool(ndc)), out.data_ptr(), _lib.stream_of(device)),
                   "nerf_amd_make_rays")
    return out


class _GetRaysFn(torch.autograd.Function):
    """get_rays with a HIP backward with respect to the pose (nerf_amd_get_rays_backward)."""

    @staticmethod
    def forward(ctx, c2w, H, W, K4):
        b = make_ray_batch(H, W, [[K4[0], 0, K4[2]], [0, K4[1], K4[3]]], c2w, 0.0, 1.0, False, False, device=c2w.device)
        ctx.meta = (H, W, K4, tuple(c2w.shape))
        return b[:, 0:3].reshape(H, W, 3), b[:, 3:6].reshape(H, W, 3)

    @staticmethod
    def backward(ctx, g_o, g_d):
        H, W, K4, shape = ctx.meta
        g_o = None if g_o is None else g_o.reshape(-1, 3).contiguous().float()
        g_d = None if g_d is None else g_d.reshape(-1, 3).contiguous().float()
        dev = (g_o if g_o is not None else g_d).device
        out = torch.empty(12, device=dev, dtype=torch.float32)
        k4 = (ctypes.c_double * 4)(*K4)
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_get_rays_backward(int(H), int(W), k4, 0, H * W, _lib.ptr(g_o), _lib.ptr(g_d),
                                                      out.data_ptr(), _lib.stream_of(dev)), "nerf_amd_get_rays_backward")
        g = torch.zeros(shape, device=dev, dtype=torch.float32)
        g[:3, :4] = out.reshape(3, 4)
        return g, None, None, None


def get_rays(H, W, K, c2w):
    """rays_o, rays_d [H, W, 3] (utils.py:33-42); pixel centres at integer coordinates, camera looks
    down -z.  Differentiable with respect to a device-resident ``c2w`` that requires grad."""
    if isinstance(c2w, torch.Tensor) and c2w.is_cuda and c2w.requires_grad and torch.is_grad_enabled():
        return _GetRaysFn.apply(c2w.float(), int(H), int(W), (float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2])))
    dev = c2w.device if isinstance(c2w, torch.Tensor) and c2w.is_cuda else _default_device()
    b = make_ray_batch(H, W, K, c2w, 0.0, 1.0, False, False, device=dev)
    return b[:, 0:3].reshape(H, W, 3), b[:, 3:6].reshape(H, W, 3)


class _RaysAtPixelsFn(torch.autograd.Function):
    """get_rays_at with a HIP backward with respect to the pose; nothing touches the host.  c2w [3|4, 4] is B = 1 of c2w
    [B, 3|4, 4]: the rank is looked at HERE (no indexing node enters the graph) and outputs and gradient have the caller's rank."""

    @staticmethod
    def forward(ctx, c2w, pix, H, W, K4):
        dev, n, lead = c2w.device, pix.shape[0], tuple(c2w.shape[:-2])
        o, d = torch.empty(*lead, n, 3, device=dev, dtype=torch.float32), torch.empty(*lead, n, 3, device=dev, dtype=torch.float32)
        k4 = (ctypes.c_double * 4)(*K4)
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_rays_at_pixels_batch(H, W, k4, c2w.data_ptr(), c2w.stride(0) if lead else 0, c2w.stride(-2),
                                                         lead[0] if lead else 1, pix.data_ptr(), n, o.data_ptr(), d.data_ptr(),
                                                         _lib.stream_of(dev)), "nerf_amd_rays_at_pixels_batch")
        ctx.meta = (H, W, K4, tuple(c2w.shape))
        ctx.pix = pix
        return o, d

    @staticmethod
    def backward(ctx, g_o, g_d):
        H, W, K4, shape = ctx.meta
        pix = ctx.pix
        dev, n = pix.device, pix.shape[0]
        g_o = None if g_o is None else g_o.contiguous().float()
        g_d = None if g_d is None else g_d.contiguous().float()
        k4 = (ctypes.c_double * 4)(*K4)
        with torch.cuda.device(dev):
            if len(shape) == 2:
                # one pose: any n (several blocks and `partials` beyond 16384).  The kernel overwrites the first 12 floats =
                # rows 0..2; row 3 of a [4, 4] pose gets no gradient
                g = torch.zeros(shape, device=dev, dtype=torch.float32) if shape[0] > 3 else torch.empty(shape, device=dev, dtype=torch.float32)
                partials = torch.empty(256 * 12, device=dev, dtype=torch.float32) if n > 16384 else None
                _lib.check(lib.nerf_amd_rays_at_pixels_backward(H, W, k4, pix.data_ptr(), n, _lib.ptr(g_o), _lib.ptr(g_d), g.data_ptr(),
                                                                _lib.ptr(partials), _lib.stream_of(dev)), "nerf_amd_rays_at_pixels_backward")
                return g, None, None, None, None
            g = torch.empty(shape[0], 3, 4, device=dev, dtype=torch.float32)
            _lib.check(lib.nerf_amd_rays_at_pixels_batch_backward(H, W, k4, pix.data_ptr(), n, shape[0], _lib.ptr(g_o), _lib.ptr(g_d),
                                                                  g.data_ptr(), _lib.stream_of(dev)),
                       "nerf_amd_rays_at_pixels_batch_backward")
        if shape[1] > 3:                           # row 3 of a [4, 4] pose gets no gradient
            rows = g
            g = torch.zeros(shape, device=dev, dtype=torch.float32)
            g[:, :3] = rows
        return g, None, None, None, None


def _device_pixels(pixels, H, W, device):
    """[n, 2] int32 (x, y) on `device`.  Host pixels (list, array, CPU tensor) are checked against the image; a device
    tensor is converted there and trusted."""
    if isinstance(pixels, torch.Tensor) and pixels.is_cuda:
        if pixels.dim() != 2 or pixels.shape[1] != 2 or pixels.is_floating_point():
            raise _lib.NerfAmdError("pixels must be an integer tensor [n, 2] of (x, y), got %s %s" % (pixels.dtype, tuple(pixels.shape)))
        return pixels.to(device=device, dtype=torch.int32).contiguous()
    host = torch.as_tensor(np.asarray(pixels) if not isinstance(pixels, torch.Tensor) else pixels)
    if host.dim() != 2 or host.shape[1] != 2 or host.is_floating_point():
        raise _lib.NerfAmdError("pixels must be integers [n, 2] of (x, y), got %s %s" % (host.dtype, tuple(host.shape)))
    if host.numel() > 0 and (int(host.min()) < 0 or int(host[:, 0].max()) >= W or int(host[:, 1].max()) >= H):
        raise _lib.NerfAmdError("pixels outside the %d x %d image (x in [0, %d), y in [0, %d))" % (H, W, W, H))
    return host.to(device=device, dtype=torch.int32).contiguous()


def get_rays_at(H, W, K, c2w, pixels):
    """rays_o, rays_d [n, 3] of the n pixels `pixels` [n, 2] = (x, y) -- column, row, as the pose-estimation demo's
    `batch` has them (demo_est_rel_pose.py:77-85): get_rays(H, W, K, c2w)[y, x] bit for bit, without generating the other
    H W - n rays.  c2w is a DEVICE tensor [3, 4] or [4, 4] and is read on the device: no host copy, no synchronisation, so
    the call can be captured in a HIP graph and sees the pose's current values on every replay (get_rays brings the pose
    to the host).  Differentiable with respect to c2w; the backward sums in a fixed order (equal inputs, equal bits).

    `pixels`: an integer device tensor (int32, or int64 converted on the device), or host integers (list, array, CPU
    tensor).  Host pixels outside the image raise NerfAmdError.  A DEVICE tensor is TRUSTED: checking it would need a
    synchronisation.  (Out-of-range values are harmless to memory -- a pixel only enters arithmetic -- and give the ray
    of that off-image position.)

    B poses at once: c2w [B, 3, 4] or [B, 4, 4] (B <= 1024) gives rays_o, rays_d [B, n, 3] at the SAME pixels, slice b
    bit-equal to get_rays_at(H, W, K, c2w[b], pixels); the backward is one block per hypothesis (n <= 16384)."""
    if not (isinstance(c2w, torch.Tensor) and c2w.is_cuda):
        raise _lib.NerfAmdError("get_rays_at reads the pose on the device: c2w must be a ROCm tensor (utils.get_rays takes host poses)")
    batch = c2w.dim() == 3
    if batch and (c2w.shape[1] not in (3, 4) or c2w.shape[2] != 4 or not 1 <= c2w.shape[0] <= POSE_BATCH_MAX):
        raise _lib.NerfAmdError("a pose batch must be [B, 3, 4] or [B, 4, 4] with 1 <= B <= %d, got %s" % (POSE_BATCH_MAX, tuple(c2w.shape)))
    if not batch and (c2w.dim() != 2 or c2w.shape[0] not in (3, 4) or c2w.shape[1] != 4):
        raise _lib.NerfAmdError("c2w must be [3, 4] or [4, 4], got %s" % (tuple(c2w.shape),))
    # already usable strides (rows of >= 4 floats with unit stride inside, poses at any non-negative distance): no copy
    usable = c2w.dtype == torch.float32 and c2w.stride(-1) == 1 and c2w.stride(-2) >= 4 and (not batch or c2w.stride(0) >= 0)
    pose = c2w if usable else c2w.float().contiguous()
    pix = _device_pixels(pixels, int(H), int(W), pose.device)
    K4 = (float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
    if not (pose.requires_grad and torch.is_grad_enabled()):
        pose = pose.detach()
    return _RaysAtPixelsFn.apply(pose, pix, int(H), int(W), K4)


class _RaysIndexedFn(torch.autograd.Function):
    """get_rays_indexed with a HIP backward with respect to the pose table (one block per pose, fixed order); pose_index None
    is the stacked-row mode of nerf_amd_rays_at_pixels_indexed."""

    @staticmethod
    def forward(ctx, c2w, pix, pose_index, H, W, K4):
        dev, n, M = c2w.device, pix.shape[0], c2w.shape[0]
        o, d = torch.empty(n, 3, device=dev, dtype=torch.float32), torch.empty(n, 3, device=dev, dtype=torch.float32)
        k4 = (ctypes.c_double * 4)(*K4)
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_rays_at_pixels_indexed(H, W, k4, c2w.data_ptr(), c2w.stride(0), c2w.stride(1), M, pix.data_ptr(),
                                                           _lib.ptr(pose_index), n, o.data_ptr(), d.data_ptr(), _lib.stream_of(dev)),
                       "nerf_amd_rays_at_pixels_indexed")
        ctx.meta = (H, W, K4, tuple(c2w.shape))
        ctx.pix, ctx.pose_index = pix, pose_index
        return o, d

    @staticmethod
    def backward(ctx, g_o, g_d):
        H, W, K4, shape = ctx.meta
        pix, pose_index = ctx.pix, ctx.pose_index
        dev = pix.device
        g_o = None if g_o is None else g_o.contiguous().float()
        g_d = None if g_d is None else g_d.contiguous().float()
        k4 = (ctypes.c_double * 4)(*K4)
        g = torch.empty(shape[0], 3, 4, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_rays_at_pixels_indexed_backward(H, W, k4, pix.data_ptr(), _lib.ptr(pose_index), pix.shape[0], shape[0],
                                                                    _lib.ptr(g_o), _lib.ptr(g_d), g.data_ptr(), _lib.stream_of(dev)),
                       "nerf_amd_rays_at_pixels_indexed_backward")
        if shape[1] > 3:                           # row 3 of a [4, 4] pose gets no gradient
            rows = g
            g = torch.zeros(shape, device=dev, dtype=torch.float32)
            g[:, :3] = rows
        return g, None, None, None, None, None


def _host_pose_index(pose_index, n, M):
    """Host pose indices (list, array, CPU tensor) as a checked int32 CPU tensor [n]: they select rows of the pose table."""
    host = torch.as_tensor(np.asarray(pose_index) if not isinstance(pose_index, torch.Tensor) else pose_index)
    if host.dim() != 1 or host.shape[0] != n or host.is_floating_point():
        raise _lib.NerfAmdError("pose_index must be %d integers (one per pixel), got %s %s" % (n, host.dtype, tuple(host.shape)))
    if host.numel() > 0 and (int(host.min()) < 0 or int(host.max()) >= M):
        raise _lib.NerfAmdError("pose_index outside [0, %d): the table holds %d poses" % (M, M))
    return host.to(torch.int32).contiguous()


def get_rays_indexed(H, W, K, c2w, pixels, pose_index=None):
    """rays_o, rays_d [n, 3] of n pixels where ray i has its OWN pose out of a table: what a training batch that mixes
    images needs when the poses are learned.  c2w is a DEVICE tensor [M, 3, 4] or [M, 4, 4] (1 <= M <= 1024), read on the
    device; row i is get_rays_at(H, W, K, c2w[p_i], pixel_i) bit for bit.

      pose_index [n] integers:  p_i = pose_index[i] and pixels [n, 2] = (x, y) in that image;
      pose_index None:          pixels [n, 2] = (x, y) address the M images stacked as one [M H, W] image (what
                                ImageBankSampler.draw() returns): p_i = y // H, the row is y - p_i H.

    Differentiable with respect to c2w: the backward is one block per pose, in a fixed order (equal inputs, equal bits), any
    n.  Same stride, dtype and device rules as get_rays_at: host pixels / indices outside the image / [0, M) raise
    NerfAmdError; DEVICE tensors are trusted (checking would synchronise) -- and harmless: a pose index outside [0, M)
    never forms an address, that ray is NaN and enters no gradient.  No host copy, no synchronisation: capturable."""
    if not isinstance(c2w, torch.Tensor) or c2w.dim() != 3 or c2w.shape[1] not in (3, 4) or c2w.shape[2] != 4 \
            or not 1 <= c2w.shape[0] <= POSE_BATCH_MAX:
        raise _lib.NerfAmdError("a pose table must be a tensor [M, 3, 4] or [M, 4, 4] with 1 <= M <= %d, got %s"
                                % (POSE_BATCH_MAX, tuple(getattr(c2w, "shape", ())) or type(c2w).__name__))
    H, W, M = int(H), int(W), c2w.shape[0]
    cpu = torch.device("cpu")
    if not (isinstance(pixels, torch.Tensor) and pixels.is_cuda):              # host inputs are checked before anything else
        pixels = _device_pixels(pixels, H if pose_index is not None else M * H, W, cpu)
    if pose_index is not None and not (isinstance(pose_index, torch.Tensor) and pose_index.is_cuda):
        pose_index = _host_pose_index(pose_index, pixels.shape[0], M)
    if not c2w.is_cuda:
        raise _lib.NerfAmdError("get_rays_indexed reads the poses on the device: c2w must be a ROCm tensor")
    usable = c2w.dtype == torch.float32 and c2w.stride(2) == 1 and c2w.stride(1) >= 4 and c2w.stride(0) >= 0
    pose = c2w if usable else c2w.float().contiguous()
    pix = _device_pixels(pixels, H, W, pose.device) if pixels.is_cuda else pixels.to(pose.device)
    if pose_index is not None:
        if pose_index.dim() != 1 or pose_index.shape[0] != pix.shape[0] or pose_index.is_floating_point():
            raise _lib.NerfAmdError("pose_index must be %d integers (one per pixel), got %s %s"
                                    % (pix.shape[0], pose_index.dtype, tuple(pose_index.shape)))
        pose_index = pose_index.to(device=pose.device, dtype=torch.int32).contiguous()
    K4 = (float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
    if not (pose.requires_grad and torch.is_grad_enabled()):
        pose = pose.detach()
    return _RaysIndexedFn.apply(pose, pix, pose_index, H, W, K4)


class _Se3Fn(torch.autograd.Function):
    """T[b] = exp_i(w[b], v[b], theta[b]) x_b (nerf_amd_se3_transform_batch): one launch forward, one backward; x is a constant.
    w, v [3] and theta [] are B = 1 of w, v [B, 3] and theta [B] (contiguous): T and the gradients have the caller's shapes."""

    @staticmethod
    def forward(ctx, w, v, theta, x):
        T = torch.empty(*theta.shape, 4, 4, device=x.device, dtype=torch.float32)
        ctx.x_stride = 16 if x.dim() == 3 else 0
        with torch.cuda.device(x.device):
            _lib.check(lib.nerf_amd_se3_transform_batch(w.data_ptr(), v.data_ptr(), theta.data_ptr(), x.data_ptr(), ctx.x_stride,
                                                        theta.numel(), T.data_ptr(), _lib.stream_of(x.device)),
                       "nerf_amd_se3_transform_batch")
        ctx.save_for_backward(w, v, theta, x)
        return T

    @staticmethod
    def backward(ctx, g_T):
        w, v, theta, x = ctx.saved_tensors
        B = theta.numel()
        g = torch.empty(7 * B, device=x.device, dtype=torch.float32)             # g_w [B, 3] | g_v [B, 3] | g_theta [B]
        g_T = g_T.contiguous().float()
        with torch.cuda.device(x.device):
            _lib.check(lib.nerf_amd_se3_transform_batch_backward(w.data_ptr(), v.data_ptr(), theta.data_ptr(), x.data_ptr(), ctx.x_stride,
                                                                 B, g_T.data_ptr(), g.data_ptr(), g.data_ptr() + 12 * B,
                                                                 g.data_ptr() + 24 * B, _lib.stream_of(x.device)),
                       "nerf_amd_se3_transform_batch_backward")
        return g[:3 * B].view(w.shape), g[3 * B:6 * B].view(v.shape), g[6 * B:].view(theta.shape), None


def _se3_apply(module, x):
    """The end of CameraTransf.forward and CameraTransfBatch.forward (x's shape is checked): the device and dtype refusals,
    then the one Function."""
    me = type(module).__name__
    _lib.require_device(x, "x")
    _lib.require_device(module.w, "%s's parameters" % me)
    if any(p.dtype != torch.float32 or p.device != x.device or not p.is_contiguous() for p in (module.w, module.v, module.theta)):
        raise _lib.NerfAmdError("%s's parameters must be contiguous fp32 on the pose's device (%s)" % (me, x.device))
    return _Se3Fn.apply(module.w, module.v, module.theta, x.detach().float().contiguous())


class CameraTransf(torch.nn.Module):
    """The pose-estimation demo's camera_transf module (demo_est_rel_pose.py:36-66): a learnable rigid motion
    exp_i(w, v, theta) applied to a start pose, T = exp_i @ x, with K = [w]x (the cross-product matrix of w):

        exp_i[:3, :3] = I + sin(theta) K + (1 - cos(theta)) K^2
        exp_i[:3, 3]  = (theta I + (1 - cos(theta)) K + (theta - sin(theta)) K^2) v            exp_i[3] = (0, 0, 0, 1)

    Same parameters (w [3], v [3], theta [], normal(0, 1e-6)), same state_dict; forward and backward are one kernel each
    (about forty scalar torch ops each way in the demo) and read everything from device memory.  x [4, 4] is a constant:
    it gets no gradient."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.normal(0., 1e-6, size=(3,)))
        self.v = torch.nn.Parameter(torch.normal(0., 1e-6, size=(3,)))
        self.theta = torch.nn.Parameter(torch.normal(0., 1e-6, size=()))

    def forward(self, x):
        if tuple(x.shape) != (4, 4):
            raise _lib.NerfAmdError("CameraTransf takes a [4, 4] pose, got %s" % (tuple(x.shape),))
        return _se3_apply(self, x)


class CameraTransfBatch(torch.nn.Module):
    """n_poses CameraTransf modules in one: w [B, 3], v [B, 3], theta [B] (normal(0, 1e-6) like CameraTransf; state_dict keys
    w, v, theta), T[b] = exp_i(w[b], v[b], theta[b]) @ x_b.  forward(x) takes one start pose [4, 4] shared by all hypotheses
    or [B, 4, 4] and returns [B, 4, 4]; row b is bit-equal to a CameraTransf with row b's parameters, forward and backward
    (one launch each, one lane per hypothesis).  x is a constant.  This is the module of multi-start pose estimation
    (CapturedMultiPoseStep): Adam is elementwise, so one optim.Adam over the three tensors is B independent Adams."""

    def __init__(self, n_poses):
        super().__init__()
        B = int(n_poses)
        if not 1 <= B <= POSE_BATCH_MAX:
            raise _lib.NerfAmdError("CameraTransfBatch holds 1..%d poses, got %d" % (POSE_BATCH_MAX, B))
        self.w = torch.nn.Parameter(torch.normal(0., 1e-6, size=(B, 3)))
        self.v = torch.nn.Parameter(torch.normal(0., 1e-6, size=(B, 3)))
        self.theta = torch.nn.Parameter(torch.normal(0., 1e-6, size=(B,)))

    @property
    def n_poses(self):
        return self.w.shape[0]

    def forward(self, x):
        B = self.n_poses
        if tuple(x.shape) not in ((4, 4), (B, 4, 4)):
            raise _lib.NerfAmdError("CameraTransfBatch(%d) takes a [4, 4] or [%d, 4, 4] pose, got %s" % (B, B, tuple(x.shape)))
        return _se3_apply(self, x)

    def pose_module(self, b):
        """A CameraTransf holding COPIES of hypothesis b's seven numbers (on their device): the way to go on with the winner
        alone in a CapturedPoseStep."""
        m = CameraTransf().to(self.w.device)
        with torch.no_grad():
            m.w.copy_(self.w[b]); m.v.copy_(self.v[b]); m.theta.copy_(self.theta[b])
        return m


class _Se3ExpFn(torch.autograd.Function):
    """T[m] = Exp(xi[m]) x_m (nerf_amd_se3_exp_batch): one launch forward, one backward; x is a constant."""

    @staticmethod
    def forward(ctx, xi, x):
        M = xi.shape[0]
        T = torch.empty(M, 4, 4, device=x.device, dtype=torch.float32)
        ctx.x_stride = 16 if x.dim() == 3 else 0
        with torch.cuda.device(x.device):
            _lib.check(lib.nerf_amd_se3_exp_batch(xi.data_ptr(), x.data_ptr(), ctx.x_stride, M, T.data_ptr(), _lib.stream_of(x.device)),
                       "nerf_amd_se3_exp_batch")
        ctx.save_for_backward(xi, x)
        return T

    @staticmethod
    def backward(ctx, g_T):
        xi, x = ctx.saved_tensors
        g = torch.empty_like(xi)
        g_T = g_T.contiguous().float()
        with torch.cuda.device(x.device):
            _lib.check(lib.nerf_amd_se3_exp_batch_backward(xi.data_ptr(), x.data_ptr(), ctx.x_stride, xi.shape[0], g_T.data_ptr(),
                                                           g.data_ptr(), _lib.stream_of(x.device)), "nerf_amd_se3_exp_batch_backward")
        return g, None


def _se3_exp(xi, x, me):
    """Exp(xi) @ x for xi [M, 6] and x [4, 4] or [M, 4, 4]: the shape, device and dtype refusals, then the one Function."""
    M = xi.shape[0]
    if tuple(x.shape) not in ((4, 4), (M, 4, 4)):
        raise _lib.NerfAmdError("%s(%d) takes a [4, 4] or [%d, 4, 4] pose, got %s" % (me, M, M, tuple(x.shape)))
    _lib.require_device(x, "x")
    _lib.require_device(xi, "%s's parameter" % me)
    if xi.dtype != torch.float32 or xi.device != x.device:
        raise _lib.NerfAmdError("%s's parameter must be fp32 on the pose's device (%s)" % (me, x.device))
    return _Se3ExpFn.apply(xi.contiguous(), x.detach().float().contiguous())


class SE3Twist(torch.nn.Module):
    """n_poses rigid corrections as se(3) twists: the parameter is xi [M, 6] = (omega, upsilon) per pose, EXACTLY ZERO at
    construction, and forward(x) = Exp(xi) @ x (include/nerf_amd.h, nerf_amd_se3_exp_batch) for one pose [4, 4] shared by all
    or [M, 4, 4]; returns [M, 4, 4].  One launch each way, one lane per pose, fp64 inside; x is a constant.

    Why not CameraTransfBatch: the demo's (w, v, theta) pose is bilinear in theta and (w, v), so at zero every derivative
    vanishes and at its normal(0, 1e-6) start every derivative is a millionth of a gradient -- tolerable for one pose and
    300 steps, wrong for hundreds of poses trained beside a field.  The twist's derivative at xi = 0 is the six generators
    applied to x, so a correction can start at "none": forward at xi = 0 returns x bit for bit."""

    def __init__(self, n_poses):
        super().__init__()
        M = int(n_poses)
        if not 1 <= M <= POSE_BATCH_MAX:
            raise _lib.NerfAmdError("SE3Twist holds 1..%d poses, got %d" % (POSE_BATCH_MAX, M))
        self.xi = torch.nn.Parameter(torch.zeros(M, 6))

    @property
    def n_poses(self):
        return self.xi.shape[0]

    def forward(self, x):
        return _se3_exp(self.xi, x, "SE3Twist")


class LearnedPoses(torch.nn.Module):
    """Camera poses that are trained beside the field: the given poses [M, 4, 4] (or [M, 3, 4]) as a buffer and an SE3Twist
    `twist`; forward() returns the current poses Exp(xi_m) @ pose_m, [M, 4, 4].  A fresh module returns the given poses bit
    for bit.  Rows listed in `frozen` always do, and their xi.grad is exactly zero (so Adam leaves them at zero): a
    reconstruction is only defined up to a rigid motion of everything, and freezing one or two views fixes that gauge.
    state_dict: poses, twist.xi."""

    def __init__(self, poses, frozen=()):
        super().__init__()
        poses = torch.as_tensor(np.asarray(poses) if not isinstance(poses, torch.Tensor) else poses).detach().float()
        if poses.dim() != 3 or tuple(poses.shape[1:]) not in ((3, 4), (4, 4)) or not 1 <= poses.shape[0] <= POSE_BATCH_MAX:
            raise _lib.NerfAmdError("LearnedPoses takes poses [M, 4, 4] or [M, 3, 4] with 1 <= M <= %d, got %s"
                                    % (POSE_BATCH_MAX, tuple(poses.shape)))
        M = poses.shape[0]
        if poses.shape[1] == 3:
            poses = torch.cat([poses, poses.new_tensor([0., 0., 0., 1.]).expand(M, 1, 4)], 1)
        frozen = sorted({int(i) for i in frozen})
        if any(not 0 <= i < M for i in frozen):
            raise _lib.NerfAmdError("frozen views %s are not all in [0, %d)" % (frozen, M))
        self.frozen = tuple(frozen)
        self.register_buffer("poses", poses.contiguous().clone())
        free = torch.ones(M, 1)
        free[list(frozen)] = 0.0
        self.register_buffer("free", free, persistent=False)       # construction-time configuration, not state
        self.twist = SE3Twist(M)

    @property
    def n_poses(self):
        return self.poses.shape[0]

    def forward(self):
        xi = self.twist.xi * self.free if self.frozen else self.twist.xi      # a frozen row: xi 0 in, gradient times 0 out
        return _se3_exp(xi, self.poses, "LearnedPoses")


# ---------------------------------------------------------------- which pixels a pose-estimation step looks at
STRATEGIES = ("random", "interest_point", "interest_region")          # the demo's --sampling_strategy values


def _sensor_image(image):
    """Shape and dtype check of a sensor image, on the host: [H, W, 3|4], uint8 or floating point; numpy array or tensor."""
    if not isinstance(image, torch.Tensor):
        image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] not in (3, 4) or image.shape[0] < 1 or image.shape[1] < 1:
        raise _lib.NerfAmdError("the sensor image must be [H, W, 3] or [H, W, 4], got %s" % (tuple(image.shape),))
    floating = image.is_floating_point() if isinstance(image, torch.Tensor) else np.issubdtype(image.dtype, np.floating)
    is_u8 = image.dtype in (torch.uint8, np.dtype(np.uint8))
    if not (floating or is_u8):
        raise _lib.NerfAmdError("the sensor image must be uint8 (0..255) or floating point (0..1), got %s" % (image.dtype,))
    return image, is_u8


def _image_u8_device(image, is_u8, device):
    """uint8 [H, W, C] contiguous on `device`; a float image goes through to8b (utils.py:30)."""
    if not is_u8:
        image = to8b(image if (isinstance(image, torch.Tensor) and image.is_cuda) else
                     (image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else image))
    return torch.as_tensor(image).to(device).contiguous()


def _host_points(points, H, W):
    """The caller's interest points [N, 2] (x, y) as a checked int64 host tensor (they address the mask)."""
    if isinstance(points, torch.Tensor):
        points = points.detach().cpu()
    pts = _device_pixels(points, H, W, torch.device("cpu"))
    if pts.shape[0] == 0:
        raise _lib.NerfAmdError("no interest points were given")
    return pts.long()


def _interest_mask(img8, quality):
    """nerf_amd_interest_points on a uint8 device image [H, W, C] -> uint8 mask [H, W]."""
    H, W, C = img8.shape
    dev = img8.device
    ws = torch.empty(int(lib.nerf_amd_interest_points_workspace(H, W)) // 8, dtype=torch.int64, device=dev)
    mask = torch.empty(H, W, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.nerf_amd_interest_points(img8.data_ptr(), H, W, C, int(quality), ws.data_ptr(), mask.data_ptr(),
                                                _lib.stream_of(dev)), "nerf_amd_interest_points")
    return mask


def _dilate_mask(mask, k, iterations):
    out = torch.empty_like(mask)
    H, W = mask.shape
    with torch.cuda.device(mask.device):
        _lib.check(lib.nerf_amd_dilate_mask(mask.data_ptr(), H, W, int(k), int(iterations), out.data_ptr(),
                                            _lib.stream_of(mask.device)), "nerf_amd_dilate_mask")
    return out


def _compact_mask(mask):
    """coords[mask]: ([M, 2] int32 (x, y) in row-major order, M).  Synchronises once, to learn M."""
    H, W = mask.shape
    dev = mask.device
    blocks = torch.empty((H * W + 255) // 256, dtype=torch.int32, device=dev)
    full = torch.empty(H * W, 2, dtype=torch.int32, device=dev)
    count = torch.empty((), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.nerf_amd_compact_mask(mask.data_ptr(), H, W, blocks.data_ptr(), full.data_ptr(), count.data_ptr(),
                                             _lib.stream_of(dev)), "nerf_amd_compact_mask")
    M = int(count)
    return full[:M].clone(), M


def find_POI(image, quality=1):
    """Interest points of a sensor image, [N, 2] int32 (x, y) in row-major order, a device tensor.

    This is a STAND-IN for the demo's find_POI (demo_est_rel_pose.py:151-164), not a reproduction of it: the demo runs cv2's
    SIFT detector, which this package neither needs nor can match.  The detector here is exact integer Harris corners
    (include/nerf_amd.h, nerf_amd_interest_points): deterministic, already de-duplicated, `quality` = the percentage of
    the strongest response a corner must reach.  With cv2 at hand, pass SIFT's points to PixelSampler(points=...) instead.
    `image`: uint8 [H, W, 3|4] (numpy or tensor); a float image in 0..1 is quantised with to8b first."""
    image, is_u8 = _sensor_image(image)
    if not 1 <= int(quality) <= 100:
        raise _lib.NerfAmdError("quality is an integer percentage, 1..100, got %r" % (quality,))
    dev = image.device if (isinstance(image, torch.Tensor) and image.is_cuda) else _default_device()
    return _compact_mask(_interest_mask(_image_u8_device(image, is_u8, dev), quality))[0]


class PixelSampler:
    """The pixel selection of the pose-estimation demo on the device: the sampling region once (demo_est_rel_pose.py:35-47),
    then per step n_rays distinct pixels of it and their colours (:75-79) in one launch with nothing on the host.

    strategy (the demo's --sampling_strategy):
      random           every pixel of the image, M = H W (no list is stored);
      interest_point   the de-duplicated interest points in row-major order;
      interest_region  the point mask dilated `dil_iter` times with a kernel_size x kernel_size window (cv2.dilate's
                       definition, exact), then coords[mask] in row-major order (exact).
    points=None finds the points with utils.find_POI (a stand-in for the demo's SIFT); otherwise `points` [N, 2] (x, y) are the
    caller's, checked on the host against the image.  H = image.shape[0], W = image.shape[1] (the demo swaps them, which only
    square images hide).  uint8 images become the demo's (img / 255.).astype(float32), a float image is taken as it is; the
    image is kept on the device as fp32 [H, W, 3] -- a fp32 device tensor whose pixels are C contiguous floats is used in place
    (a view with a row stride or a fourth channel included), so it can be rewritten between draws.

    draw() -> (pixels [n_rays, 2] int32 (x, y), target [n_rays, 3] fp32): the SAME two device tensors on every call, filled by
    nerf_amd_draw_pixels -- no synchronisation, no allocation, capturable in torch.cuda.graph.  The draw is a keyed bijection
    of [0, M) (defined in include/nerf_amd.h) of `seed` and the device counter `draw_count`, which every draw advances by one
    on the device: draw k of a seed is always the same pixels, whether eager or replayed.  The key uses the low 32 bits of
    the counter, so draws 2^32 apart repeat.  reset(count) sets the counter.  `region` is the [M, 2] list (None for random).
    Construction synchronises once to learn M and raises NerfAmdError without interest points or with n_rays > M."""

    def __init__(self, image, n_rays, strategy='interest_region', points=None, kernel_size=5, dil_iter=3, seed=0, device=None):
        if strategy not in STRATEGIES:
            raise _lib.NerfAmdError("unknown sampling strategy %r (one of %s)" % (strategy, ", ".join(STRATEGIES)))
        image, is_u8 = _sensor_image(image)
        H, W = int(image.shape[0]), int(image.shape[1])
        if int(n_rays) < 1 or int(kernel_size) < 1 or int(dil_iter) < 1:
            raise _lib.NerfAmdError("n_rays, kernel_size and dil_iter must be at least 1")
        pts = _host_points(points, H, W) if (points is not None and strategy != "random") else None
        if device is None:
            device = image.device if (isinstance(image, torch.Tensor) and image.is_cuda) else _default_device()
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.NerfAmdError("PixelSampler draws on a ROCm device, got %s -- there is no CPU path" % dev)
        self.H, self.W, self.n_rays, self.strategy, self.seed = H, W, int(n_rays), strategy, int(seed) & 0xffffffff
        self.region = None
        self.M = H * W
        if strategy != "random":
            if pts is None:
                mask = _interest_mask(_image_u8_device(image, is_u8, dev), 1)
            else:
                mask = torch.zeros(H, W, dtype=torch.uint8, device=dev)
                pts = pts.to(dev)
                mask[pts[:, 1], pts[:, 0]] = 1
            if strategy == "interest_region":
                mask = _dilate_mask(mask, kernel_size, dil_iter)
            self.region, self.M = _compact_mask(mask)
            if self.M == 0:
                raise _lib.NerfAmdError("the image has no interest points (a featureless image?): use strategy='random' or pass points=")
        if self.n_rays > self.M:
            raise _lib.NerfAmdError("cannot draw %d distinct pixels out of %d (np.random.choice(replace=False) raises too)"
                                    % (self.n_rays, self.M))
        if is_u8:                                  # the 256 values of (img / 255.).astype(float32), computed as the demo does
            lut = torch.from_numpy((np.arange(256) / 255.).astype(np.float32)).to(dev)
            self.image = lut[torch.as_tensor(image).to(dev)[..., :3].long()].contiguous()
        else:
            img = torch.as_tensor(image).to(dev)
            C = img.shape[2]
            in_place = (img.dtype == torch.float32 and img.stride(2) == 1 and img.stride(1) == C and img.stride(0) >= W * C
                        and img.data_ptr() % 4 == 0)
            self.image = img.detach() if in_place else img.detach()[..., :3].float().contiguous()
        self.draw_count = torch.zeros((), dtype=torch.int64, device=dev)
        self.pixels = torch.zeros(self.n_rays, 2, dtype=torch.int32, device=dev)
        self.target = torch.zeros(self.n_rays, 3, dtype=torch.float32, device=dev)

    def draw(self):
        dev = self.pixels.device
        img = self.image
        with torch.cuda.device(dev):
            _lib.check(lib.nerf_amd_draw_pixels(self.M, self.n_rays, self.seed, self.draw_count.data_ptr(), _lib.ptr(self.region),
                                                self.H, self.W, img.data_ptr(), img.stride(0), img.shape[2], self.pixels.data_ptr(),
                                                self.target.data_ptr(), _lib.stream_of(dev)), "nerf_amd_draw_pixels")
        return self.pixels, self.target

    def reset(self, count=0):
        """The next draw is draw `count` (a device write, stream-ordered; no synchronisation)."""
        self.draw_count.fill_(int(count))


class ImageBankSampler:
    """Training batches drawn from the images themselves: PixelSampler's 'random' draw over a bank of M images [M, H, W, 3|4]
    viewed as ONE [M H, W, C] image -- the same keyed draw, no new RNG, and no copy where the layout allows (a contiguous
    fp32 device bank is used in place).  draw() -> (pixels [n_rays, 2] int32, target [n_rays, 3] fp32): n_rays distinct
    pixels of the whole bank, (x, y) with y a row of the STACKED image, which is what get_rays_indexed(..., pose_index=None)
    takes: image y // H, row y % H.  The bank costs 12 B per pixel (fp32 RGB) where pre-computed rays cost 72 B (origin,
    direction, colour), and the rays follow the poses as they are learned.  M, H, W, n_rays, draw_count, reset(count),
    pixels and target as PixelSampler has them.  M H W <= 2^31 - 1."""

    def __init__(self, images, n_rays, seed=0, device=None):
        if not isinstance(images, torch.Tensor):
            images = np.asarray(images)
        if images.ndim != 4 or images.shape[3] not in (3, 4) or min(images.shape[:3]) < 1:
            raise _lib.NerfAmdError("the image bank must be [M, H, W, 3] or [M, H, W, 4], got %s" % (tuple(images.shape),))
        M, H, W, C = (int(s) for s in images.shape)
        if M * H * W > 0x7fffffff:
            raise _lib.NerfAmdError("the bank holds %d x %d x %d = %d pixels; one draw addresses at most 2^31 - 1" % (M, H, W, M * H * W))
        self.M, self.H, self.W = M, H, W
        self._sampler = PixelSampler(images.reshape(M * H, W, C), n_rays, strategy="random", seed=seed, device=device)
        self.n_rays, self.seed = self._sampler.n_rays, self._sampler.seed

    pixels = property(lambda self: self._sampler.pixels)
    target = property(lambda self: self._sampler.target)
    draw_count = property(lambda self: self._sampler.draw_count)
    image = property(lambda self: self._sampler.image)

    def draw(self):
        return self._sampler.draw()

    def reset(self, count=0):
        self._sampler.reset(count)


def get_rays_np(H, W, K, c2w):
    """numpy twin used by the reference's training-data batching (utils.py:45-52)."""
    i, j = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing='xy')
    dirs = np.stack([(i - K[0][2]) / K[0][0], -(j - K[1][2]) / K[1][1], -np.ones_like(i)], -1)
    rays_d = np.sum(dirs[..., np.newaxis, :] * c2w[:3, :3], -1)
    rays_o = np.broadcast_to(c2w[:3, -1], np.shape(rays_d))
    return rays_o, rays_d


def _ndc_forward(H, W, focal, near, o, d):
    oo, od = torch.empty_like(o), torch.empty_like(d)
    with torch.cuda.device(d.device):
        _lib.check(lib.nerf_amd_ndc_rays(int(H), int(W), float(focal), float(near), o.data_ptr(), d.data_ptr(),
                                         o.shape[0], oo.data_ptr(), od.data_ptr(), _lib.stream_of(d.device)),
                   "nerf_amd_ndc_rays")
    return oo, od


class _NdcRaysFn(torch.autograd.Function):
    """ndc_rays with gradients with respect to the rays (nerf_amd_ndc_rays_backward)."""

    @staticmethod
    def forward(ctx, o, d, H, W, focal, near):
        ctx.save_for_backward(o, d)
        ctx.args = (int(H), int(W), float(focal), float(near))
        return _ndc_forward(H, W, focal, near, o, d)

    @staticmethod
    def backward(ctx, g_oo, g_od):
        o, d = ctx.saved_tensors
        H, W, focal, near = ctx.args
        g_oo = None if g_oo is None else g_oo.contiguous().float()
        g_od = None if g_od is None else g_od.contiguous().float()
        g_o, g_d = torch.empty_like(o), torch.empty_like(d)
        with torch.cuda.device(d.device):
            _lib.check(lib.nerf_amd_ndc_rays_backward(H, W, focal, near, o.data_ptr(), d.data_ptr(), _lib.ptr(g_oo), _lib.ptr(g_od),
                                                      o.shape[0], g_o.data_ptr(), g_d.data_ptr(), _lib.stream_of(d.device)),
                       "nerf_amd_ndc_rays_backward")
        return g_o, g_d, None, None, None, None


def ndc_rays(H, W, focal, near, rays_o, rays_d):
    """Forward-facing NDC warp of explicit rays (utils.py:54-71).  Differentiable with respect to the rays."""
    _lib.require_device(rays_d, "rays_d")
    shape = rays_d.shape
    if torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad):
        o = rays_o.expand(shape).reshape(-1, 3).contiguous().float()
        d = rays_d.reshape(-1, 3).contiguous().float()
        oo, od = _NdcRaysFn.apply(o, d, H, W, focal, near)
    else:
        o = rays_o.detach().expand(shape).reshape(-1, 3).contiguous().float()
        d = rays_d.detach().reshape(-1, 3).contiguous().float()
        oo, od = _ndc_forward(H, W, focal, near, o, d)
    return oo.reshape(shape), od.reshape(shape)


def sample_pdf(bins, weights, N_samples, det=False, pytest=False):
    """Inverse-CDF sampling along each ray (utils.py:74-117).
    bins [R, M], weights [R, M-1] -> samples [R, N_samples]."""
    _lib.require_device(bins, "bins")
    dev = bins.device
    lead = list(bins.shape[:-1])
    b = bins.detach().reshape(-1, bins.shape[-1]).contiguous().float()
    w = weights.detach().reshape(-1, weights.shape[-1]).contiguous().float()
    if w.shape[-1] != b.shape[-1] - 1 or w.shape[0] != b.shape[0]:
        raise _lib.NerfAmdError("weights must be [..., len(bins)-1]")
    R = b.shape[0]
    u = t_lin = None
    if pytest:
        np.random.seed(0)
        if det:
            un = np.broadcast_to(np.linspace(0., 1., N_samples), [R, N_samples])
        else:
            un = np.random.rand(R, N_samples)
        u = torch.Tensor(np.ascontiguousarray(un)).to(dev)
    elif det:
        t_lin = torch.linspace(0., 1., steps=N_samples, device=dev)
    else:
        u = torch.rand([R, N_samples], device=dev)
    out = torch.empty(R, N_samples, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(lib.nerf_amd_sample_pdf(b.data_ptr(), w.data_ptr(), _lib.ptr(u), _lib.ptr(t_lin), R,
                                           b.shape[-1], int(N_samples), out.data_ptr(), _lib.stream_of(dev)),
                   "nerf_amd_sample_pdf")
    return out.reshape(lead + [N_samples])


# ---------------------------------------------------------------- factories (utils.py:119-161)
_FIELD_SKIPS = [4]          # the reference hard-codes the skip layer (utils.py:122)


def create_nerf_models(args, device=None):
    """(coarse_model, fine_model) for an args namespace, what utils.py:119-139 builds: one field, or two when
    N_importance > 0 (then both emit 5 channels); the fine field takes its depth / width from
    netdepth_fine / netwidth_fine.  fine_model is None without importance sampling."""
    from . import nerf
    device = device or _default_device()
    two_pass = args.N_importance > 0
    shared = dict(output_ch=5 if two_pass else 4, skips=list(_FIELD_SKIPS), use_viewdirs=args.use_viewdirs,
                  multires=args.multires, multires_views=args.multires_views, i_embed=args.i_embed)
    sizes = [(args.netdepth, args.netwidth)] + ([(args.netdepth_fine, args.netwidth_fine)] if two_pass else [])
    fields = [nerf.NeRF(D=depth, W=width, **shared).to(device) for depth, width in sizes]
    return fields[0], (fields[1] if two_pass else None)


def get_renderer(args, bds_dict):
    """Renderer for an args namespace and the scene's {'near', 'far'} (utils.py:141-161).  NDC rays are used
    for forward-facing LLFF scenes only, and not when args.no_ndc asks for world-space sampling."""
    from . import render_utils
    ndc = args.dataset_type == 'llff' and not args.no_ndc
    if not ndc:
        print('Not ndc!')
    return render_utils.Renderer(perturb=args.perturb, N_importance=args.N_importance, N_samples=args.N_samples,
                                 use_viewdirs=args.use_viewdirs, white_bkgd=args.white_bkgd,
                                 raw_noise_std=args.raw_noise_std, ndc=ndc, lindisp=args.lindisp, **bds_dict)


# ---------------------------------------------------------------- optimizer + checkpoints (utils.py:163-214, 444-456)
def get_optimizer(coarse_model, fine_model, args):
    """Adam over both models' parameters, lr = args.lrate (utils.py:163-172).  With the parameters on the GPU this is
    `nerf_shared_amd.optim.Adam`: a torch.optim.Adam (same state, same checkpoints) whose step is one kernel launch for
    all 48 tensors -- the 1024-ray training step is host-bound otherwise.  CPU parameters get the plain torch optimizer."""
    params = list(coarse_model.parameters())
    if fine_model is not None:
        params += list(fine_model.parameters())
    if len(params) > 0 and all(p.is_cuda for p in params):
        from . import optim
        return optim.Adam(params=params, lr=args.lrate, betas=(0.9, 0.999))
    return torch.optim.Adam(params=params, lr=args.lrate, betas=(0.9, 0.999))


def _capture_step(body, optimizer, params, repack_models, dev, warmup):
    """Warm `body` up on a side stream, capture it in a HIP graph, and put the training state back: constructing a captured
    step must not train.  The warm-up steps (which the capture needs -- lazy allocations, the optimizer's per-group fast
    path) run on the caller's placeholder inputs; parameters, moments and step counts are restored afterwards.
    `repack_models`: models whose parameters the step updates (the re-pack belongs inside the captured step)."""
    snapshot = optimizer.snapshot_training_state(params)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for i in range(max(1, warmup)):          # (the first step also establishes the optimizer's per-group fast path)
            body()
            if i == 0:
                optimizer.enable_device_scalars()
    torch.cuda.current_stream(dev).wait_stream(side)
    for m in repack_models:
        if m is not None:
            m.weights_changed()                   # the re-pack of the parameters belongs inside the captured step
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    optimizer.restore_training_state(params, snapshot)
    return graph


class _CapturedStep:
    """What the captured steps share: the optimizer they accept, and a call's tail (learning rate, replay, stale weights).
    A subclass sets self.graph (from _capture_step) and self.loss (in its captured body)."""

    _ADAM_OVER = "(utils.get_optimizer)"          # where the message says the optimizer comes from

    def _take_optimizer(self, optimizer):
        from . import optim
        if not isinstance(optimizer, optim.Adam):
            raise _lib.NerfAmdError("%s needs nerf_shared_amd.optim.Adam %s: torch's optimizers pass step-dependent scalars as "
                                    "kernel arguments, which a graph would freeze" % (type(self).__name__, self._ADAM_OVER))
        self.optimizer = optimizer
        self.params = [p for g in optimizer.param_groups for p in g["params"]]
        self._lr = None

    def _replay(self):
        lr = tuple(float(g["lr"]) for g in self.optimizer.param_groups)
        if lr != self._lr:
            self.optimizer.sync_lr()
            self._lr = lr
        self.graph.replay()
        self.optimizer.note_replayed_step()
        return self.loss


class CapturedTrainStep(_CapturedStep):
    """One iteration of the reference's training loop (main.py:77-104: render_from_rays -> img2mse(rgb) [+ img2mse(rgb0)]
    -> loss.backward() -> optimizer.step()) captured once in a HIP graph and replayed.

    The eager step costs about a hundred kernel launches; at the reference's batch size (N_rand = 1024) Python and the
    runtime spend as long enqueueing them as the GPU spends executing them.  A replay is one call.  What keeps the loop's
    semantics between replays:
      * rays / target are copied into the capture's input buffers on every call (any N_rand-ray batch of the same shape);
      * the learning rate is read from device memory: change optimizer.param_groups[i]['lr'] as main.py:108-112 does and the
        next call picks it up; the optimizer's step count advances on the device and is mirrored on the host;
      * gradients are left in `.grad` after every call (the captured step starts from zeroed gradients, like
        optimizer.zero_grad() at the top of the loop body);
      * random draws (perturb, raw_noise_std) advance with every replay (torch's graph-safe generator offsets);
      * every replay marks the stepped models' packed weights stale (optimizer.note_replayed_step()), so an eager render
        between calls (main.py's i_img / i_testset) sees the latest step.  A graph captured by hand around
        optimizer.step() must do the same after each replay: optimizer.note_replayed_step(), or model.weights_changed().
    Everything the step touches must stay alive and in place (models, optimizer state).  Needs nerf_shared_amd.optim.Adam
    (utils.get_optimizer) and models the training kernels cover.  Constructing it leaves parameters, moments and step
    counts as they were (the warm-up steps the capture needs are undone).
    The step captures whatever the renderer does: with renderer.train_occupancy set (occupancy.TrainCull) it is captured
    culled -- the fractions (the lists' capacities) are FROZEN at capture, the grid's bits are READ AT REPLAY, so
    OccupancyGrid.refresh_from_density between replays is seen by the next one; the warm-up steps of the construction add
    to the TrainCull's running totals.  Construct it with no autograd graph over the parameters alive (no render result of
    an earlier eager step in a variable): such a graph pins the parameters' gradient accumulators to the stream it ran on.

        step = utils.CapturedTrainStep(renderer, H, W, K, chunk, coarse, fine, optimizer, N_rand)
        for i in range(n_iters):
            rays, target = sample_random_ray_batch(...)          # [2, N_rand, 3], [N_rand, 3]
            loss = step(rays, target)                            # device scalar; step.psnr likewise
            for g in optimizer.param_groups: g['lr'] = new_lrate
    """

    def __init__(self, renderer, H, W, K, chunk, coarse_model, fine_model, optimizer, n_rays, warmup=3):
        self._take_optimizer(optimizer)
        dev = next(coarse_model.parameters()).device
        self.renderer, self.models = renderer, (coarse_model, fine_model)
        self.args = (H, W, K, chunk)
        self.rays = torch.zeros(2, n_rays, 3, device=dev)
        self.rays[1, :, 2] = -1.0                     # a valid placeholder batch for the warm-up (zero directions have no unit vector)
        self.target = torch.full((n_rays, 3), 0.5, device=dev)
        self.loss = self.psnr = None
        self.graph = _capture_step(self._body, optimizer, self.params, self.models, dev, warmup)

    def _body(self):
        H, W, K, chunk = self.args
        coarse, fine = self.models
        for p in self.params:
            p.grad = None
        rgb, disp, acc, extras = self.renderer.render_from_rays(H, W, K, chunk, self.rays, coarse, fine, retraw=True)
        loss = img2mse(rgb, self.target)
        self.psnr = -10. * torch.log(loss.detach()) / math.log(10.)       # mse2psnr without its host-side constant tensor
        if 'rgb0' in extras:
            loss = loss + img2mse(extras['rgb0'], self.target)
        loss.backward()
        self.optimizer.step()
        self.loss = loss.detach()

    def __call__(self, rays, target):
        self.rays.copy_(rays if isinstance(rays, torch.Tensor) else torch.stack(list(rays), 0), non_blocking=True)
        self.target.copy_(target, non_blocking=True)
        return self._replay()


class CapturedPoseStep(_CapturedStep):
    """One iteration of the pose-estimation demo's loop (demo_est_rel_pose.py:74-98) captured once in a HIP graph and replayed:

        pose = cam_transf(start_pose) -> get_rays_at(H, W, K, pose, pixels) -> render_from_rays -> img2mse(rgb, target)
        -> loss.backward() -> optimizer.step()

    with frozen fields and the seven numbers of a utils.CameraTransf as the only parameters.  Nothing in the body touches
    the host: the pose goes from the se(3) kernel to the ray kernel in device memory, the fields' backward is the
    inputs-only one (no weight-gradient launches), and the optimizer reads its step count and learning rate on the device.
    Between replays, as in CapturedTrainStep:
      * pixels [n_rays, 2] = (x, y) and target [n_rays, 3] are copied into the capture's input buffers on every call (device
        or host tensors; device pixels are trusted, see get_rays_at);
      * change optimizer.param_groups[i]['lr'] (the demo's lrate * 0.8 ** ((k + 1) / 100)) and the next call picks it up;
      * random draws (perturb, raw_noise_std) advance with every replay;
      * gradients of the seven parameters are left in `.grad` after every call.
    `step.pose` is the [4, 4] pose AFTER the last replay's update (cam_transf(start_pose) on the stepped parameters, what
    the demo prints and compares), a device tensor that the next replay overwrites.  Needs nerf_shared_amd.optim.Adam over
    cam_transf.parameters() and frozen models (requires_grad_(False)): a field that asked for parameter gradients would
    take the training backward for gradients nobody steps.  Constructing it leaves the seven parameters, the moments and
    the step count as they were.
    With renderer.train_occupancy set (occupancy.TrainCull) the step is captured culled, as CapturedTrainStep is: the
    fractions are frozen at capture, the grid's bits are read at replay.

        cam = utils.CameraTransf().to(device)
        opt = optim.Adam(cam.parameters(), lr=lrate, betas=(0.9, 0.999))
        step = utils.CapturedPoseStep(renderer, H, W, K, chunk, coarse, fine, cam, start_pose, opt, n_rays)
        for k in range(n_iters):
            loss = step(pixels_k, target_k)                      # device scalar
            for g in opt.param_groups: g['lr'] = lrate * 0.8 ** ((k + 1) / 100)

    With sampler=utils.PixelSampler(image, n_rays, ...) the captured body BEGINS with sampler.draw(): every replay draws its own
    n_rays pixels and gathers their colours on the device, step.pixels / step.target are the sampler's buffers (the batch of
    the last replay), and step() takes no arguments -- the loop touches the host for the learning-rate write alone.  The
    warm-up draws of the construction do not count: sampler.draw_count is afterwards what it was before.
    """

    _ADAM_OVER = "over cam_transf.parameters()"

    def __init__(self, renderer, H, W, K, chunk, coarse_model, fine_model, cam_transf, start_pose, optimizer, n_rays, warmup=3,
                 sampler=None):
        me = type(self).__name__                  # (CapturedMultiPoseStep shares this constructor)
        self._take_optimizer(optimizer)
        for name, m in (("coarse_model", coarse_model), ("fine_model", fine_model)):
            if m is not None and any(p.requires_grad for p in m.parameters()):
                raise _lib.NerfAmdError("%s optimises the pose against FROZEN fields: call %s.requires_grad_(False) "
                                        "(its parameters ask for gradients that this step would compute and nobody would use)" % (me, name))
        mine = {id(p) for p in cam_transf.parameters()}
        if not self.params or {id(p) for p in self.params} != mine:
            raise _lib.NerfAmdError("%s: the optimizer must hold exactly cam_transf's parameters (w, v, theta)" % me)
        dev = self.params[0].device
        _lib.require_device(self.params[0], "cam_transf's parameters")
        self.renderer, self.models, self.cam_transf = renderer, (coarse_model, fine_model), cam_transf
        self.args = (int(H), int(W), K, chunk)
        self.start_pose = torch.as_tensor(start_pose, dtype=torch.float32).to(dev).contiguous().clone()
        self._check_start_pose()
        self.sampler = sampler
        if sampler is not None:
            if not isinstance(sampler, PixelSampler) or sampler.pixels.device != dev:
                raise _lib.NerfAmdError("sampler must be a utils.PixelSampler on the parameters' device (%s)" % dev)
            if sampler.n_rays != int(n_rays) or (sampler.H, sampler.W) != (int(H), int(W)):
                raise _lib.NerfAmdError("the sampler draws %d pixels of a %d x %d image; this step was asked for %d rays of %d x %d"
                                        % (sampler.n_rays, sampler.H, sampler.W, int(n_rays), int(H), int(W)))
            self.pixels, self.target = sampler.pixels, sampler.target
            draws_before = sampler.draw_count.clone()
        else:
            # a valid placeholder batch for the warm-up: pixel (0, 0) n_rays times, a grey target
            self.pixels = torch.zeros(n_rays, 2, device=dev, dtype=torch.int32)
            self.target = torch.full((n_rays, 3), 0.5, device=dev)
        self.loss = self.pose = None
        self.graph = _capture_step(self._body, optimizer, self.params, (), dev, warmup)
        if sampler is not None:
            sampler.draw_count.copy_(draws_before)                # the warm-up draws do not count
        with torch.no_grad():
            self.pose.copy_(cam_transf(self.start_pose))          # (the capture left the pose of its own last update there)

    def _check_start_pose(self):
        if tuple(self.start_pose.shape) != (4, 4):
            raise _lib.NerfAmdError("start_pose must be [4, 4], got %s" % (tuple(self.start_pose.shape),))

    def _body(self):
        H, W, K, chunk = self.args
        coarse, fine = self.models
        for p in self.params:
            p.grad = None
        if self.sampler is not None:
            self.sampler.draw()                   # fills self.pixels / self.target (the sampler's buffers)
        pose = self.cam_transf(self.start_pose)
        rays_o, rays_d = get_rays_at(H, W, K, pose, self.pixels)
        rgb, disp, acc, extras = self.renderer.render_from_rays(H, W, K, chunk, self._renderer_rays(rays_o, rays_d), coarse, fine,
                                                                retraw=True)
        self.loss = self._loss_backward(rgb)
        self.optimizer.step()
        with torch.no_grad():
            self.pose = self.cam_transf(self.start_pose)

    # what differs between one pose and B hypotheses in the body: the rays' shape for the renderer, and the loss
    def _renderer_rays(self, rays_o, rays_d):
        return torch.stack([rays_o, rays_d], 0)

    def _loss_backward(self, rgb):
        loss = img2mse(rgb, self.target)          # the demo's loss is the fine pass alone (demo_est_rel_pose.py:92)
        loss.backward()
        return loss.detach()

    def __call__(self, pixels=None, target=None):
        H, W = self.args[0], self.args[1]
        if self.sampler is not None:
            if pixels is not None or target is not None:
                raise _lib.NerfAmdError("this step draws its own pixels (sampler=...): call step() without arguments")
        else:
            if pixels is None or target is None:
                raise _lib.NerfAmdError("step(pixels, target): a step built without a sampler needs both")
            pix = pixels if (isinstance(pixels, torch.Tensor) and pixels.is_cuda) else _device_pixels(pixels, H, W, self.pixels.device)
            self.pixels.copy_(pix, non_blocking=True)
            self.target.copy_(target, non_blocking=True)
        return self._replay()


class CapturedMultiPoseStep(CapturedPoseStep):
    """CapturedPoseStep for B pose hypotheses in ONE captured step (multi-start pose estimation: photometric refinement has
    a narrow basin, so the loop is run from several starts and the best is kept):

        [sampler.draw()] -> poses = cam_transfs(start_poses) [B, 4, 4] -> get_rays_at(H, W, K, poses, pixels) [B, n, 3] x 2
        -> render_from_rays(rays [2, B n, 3], hypothesis-major rows) -> losses = img2mse_each(rgb.view(B, n, 3), target) [B]
        -> losses.sum().backward() -> optimizer.step()

    To every field kernel the B hypotheses are one batch of B n rays.  The loss is the SUM over hypotheses, so hypothesis b's
    gradient is exactly what it would get alone, and Adam is elementwise, so one optim.Adam over the three [B, ...] tensors
    of a utils.CameraTransfBatch is B independent Adams with a common step count and learning rate.  The pixels (and target)
    are SHARED by all hypotheses: that makes their losses comparable and lets one sampler.draw() feed all of them.

    Same contracts as CapturedPoseStep (frozen models, optim.Adam over exactly cam_transfs.parameters(), construction leaves
    parameters, moments, step count and sampler.draw_count as they were, the learning rate is picked up from param_groups,
    step(pixels, target) or step() with a sampler).  start_poses is [B, 4, 4], or one [4, 4] for all (then the hypotheses
    differ by the module rows the caller sets).  step() returns `step.losses` [B]; `step.poses` [B, 4, 4] are the poses AFTER
    the update; both are device tensors that the next replay overwrites.  The whole body runs on the capturing stream.  With
    chunk < B n the renderer's chunk loop runs (correct, pointless): pass chunk >= B n.

        cams = utils.CameraTransfBatch(B).to(device)
        opt = optim.Adam(cams.parameters(), lr=lrate, betas=(0.9, 0.999))
        step = utils.CapturedMultiPoseStep(renderer, H, W, K, B * n_rays, coarse, fine, cams, start_poses, opt, n_rays, sampler=s)
        for k in range(n_iters):
            losses = step()                                      # [B], device
            for g in opt.param_groups: g['lr'] = lrate * 0.8 ** ((k + 1) / 100)
        winner = cams.pose_module(int(best))                     # go on alone in a CapturedPoseStep
    """

    cam_transfs = property(lambda self: self.cam_transf)
    start_poses = property(lambda self: self.start_pose)
    losses = property(lambda self: self.loss)
    poses = property(lambda self: self.pose)

    def _check_start_pose(self):
        if not isinstance(self.cam_transf, CameraTransfBatch):
            raise _lib.NerfAmdError("CapturedMultiPoseStep steps a utils.CameraTransfBatch, got %s" % type(self.cam_transf).__name__)
        B = self.cam_transf.n_poses
        if tuple(self.start_pose.shape) not in ((4, 4), (B, 4, 4)):
            raise _lib.NerfAmdError("start_poses must be [%d, 4, 4] (the module's hypotheses) or [4, 4], got %s"
                                    % (B, tuple(self.start_pose.shape)))

    def _renderer_rays(self, rays_o, rays_d):     # [B, n, 3] each -> hypothesis-major rows
        Bn = self.cam_transf.n_poses * self.pixels.shape[0]
        return torch.stack([rays_o.view(Bn, 3), rays_d.view(Bn, 3)], 0)

    def _loss_backward(self, rgb):
        losses = img2mse_each(rgb.reshape(self.cam_transf.n_poses, self.pixels.shape[0], 3), self.target)
        losses.sum().backward()
        return losses.detach()


class CapturedJointStep(_CapturedStep):
    """CapturedTrainStep with LEARNED camera poses (BARF / iMAP-style mapping: every training image has its own correctable
    pose), captured once in a HIP graph and replayed:

        [sampler.draw()] -> poses = learned_poses() [M, 4, 4] -> get_rays_indexed(H, W, K, poses, pixels, pose_index)
        -> render_from_rays -> img2mse(rgb) [+ img2mse(rgb0)] -> loss.backward() -> optimizer.step()

    The fields' training backward returns parameter gradients and ray gradients from one call; the ray gradients go through
    the indexed ray kernel (one block per pose, fixed order) and the twist kernel to learned_poses.twist.xi.  The optimizer
    is ONE optim.Adam whose parameter groups hold the field parameters and xi, each with its own learning rate:

        poses = utils.LearnedPoses(noisy_poses, frozen=(0,)).to(device)
        opt = optim.Adam([{"params": field_params, "lr": lrate}, {"params": [poses.twist.xi], "lr": pose_lr}], betas=(0.9, 0.999))
        bank = utils.ImageBankSampler(images, N_rand)                                   # [M, H, W, 3] on the device
        step = utils.CapturedJointStep(renderer, H, W, K, chunk, coarse, fine, poses, opt, N_rand, sampler=bank)
        for i in range(n_iters):
            loss = step()                                        # device scalar; step.psnr, step.poses [M, 4, 4] likewise
            opt.param_groups[0]['lr'] = new_lrate                # read at the next replay, per group

    Without a sampler, step(pixels, pose_index, target) copies pixels [n_rays, 2] = (x, y), pose_index [n_rays] and target
    [n_rays, 3] into the capture's buffers (host values are checked against the image and [0, M); device tensors are
    trusted, see get_rays_indexed).  `step.poses` is learned_poses() AFTER the update, `step.loss` / `step.psnr` are as in
    CapturedTrainStep; all are device tensors that the next replay overwrites.  Same contracts as CapturedTrainStep
    otherwise: construction leaves parameters, moments, step counts and sampler.draw_count as they were; the renderer is
    captured as it is (ray bounds, train_occupancy and NDC carry ray gradients).  Refused: an optimizer without xi or with
    tensors that are neither xi nor a field parameter, and FROZEN fields -- poses against frozen fields are
    CapturedMultiPoseStep's case (inputs-only backward, no weight-gradient launches)."""

    _ADAM_OVER = "over the field parameters and learned_poses.twist.xi"

    def __init__(self, renderer, H, W, K, chunk, coarse_model, fine_model, learned_poses, optimizer, n_rays, warmup=3, sampler=None):
        self._take_optimizer(optimizer)
        if not isinstance(learned_poses, LearnedPoses):
            raise _lib.NerfAmdError("CapturedJointStep trains a utils.LearnedPoses, got %s" % type(learned_poses).__name__)
        field = [p for m in (coarse_model, fine_model) if m is not None for p in m.parameters()]
        if not field or not all(p.requires_grad for p in field):
            raise _lib.NerfAmdError("CapturedJointStep trains the fields AND the poses; with frozen fields (requires_grad_(False)) "
                                    "use utils.CapturedMultiPoseStep, whose backward skips the weight gradients")
        xi = learned_poses.twist.xi
        held = {id(p) for p in self.params}
        if id(xi) not in held:
            raise _lib.NerfAmdError("CapturedJointStep: the optimizer must hold learned_poses.twist.xi (a parameter group of its own, "
                                    "with the pose learning rate)")
        if not held <= {id(xi)} | {id(p) for p in field}:
            raise _lib.NerfAmdError("CapturedJointStep: the optimizer holds tensors that are neither field parameters nor "
                                    "learned_poses.twist.xi")
        H, W, n_rays, M = int(H), int(W), int(n_rays), learned_poses.n_poses
        if sampler is not None:
            if not isinstance(sampler, ImageBankSampler):
                raise _lib.NerfAmdError("sampler must be a utils.ImageBankSampler (a PixelSampler draws from ONE image)")
            if (sampler.M, sampler.H, sampler.W, sampler.n_rays) != (M, H, W, n_rays):
                raise _lib.NerfAmdError("the sampler draws %d pixels of %d images of %d x %d; this step was asked for %d rays of %d "
                                        "poses of %d x %d" % (sampler.n_rays, sampler.M, sampler.H, sampler.W, n_rays, M, H, W))
        _lib.require_device(xi, "learned_poses")
        dev = xi.device
        if any(p.device != dev for p in field) or (sampler is not None and sampler.pixels.device != dev):
            raise _lib.NerfAmdError("CapturedJointStep: fields, poses and sampler must be on one device (%s)" % dev)
        self.renderer, self.models, self.learned_poses, self.sampler = renderer, (coarse_model, fine_model), learned_poses, sampler
        self.args = (H, W, K, chunk)
        if sampler is not None:
            self.pixels, self.target, self.pose_index = sampler.pixels, sampler.target, None     # stacked rows name the image
            draws_before = sampler.draw_count.clone()
        else:
            # a valid placeholder batch for the warm-up: pixel (0, 0) of image 0 n_rays times, a grey target
            self.pixels = torch.zeros(n_rays, 2, device=dev, dtype=torch.int32)
            self.pose_index = torch.zeros(n_rays, device=dev, dtype=torch.int32)
            self.target = torch.full((n_rays, 3), 0.5, device=dev)
        self.loss = self.psnr = self.poses = None
        self.graph = _capture_step(self._body, optimizer, self.params, self.models, dev, warmup)
        if sampler is not None:
            sampler.draw_count.copy_(draws_before)                # the warm-up draws do not count
        with torch.no_grad():
            self.poses.copy_(learned_poses())                     # (the capture left the poses of its own last update there)

    def _body(self):
        H, W, K, chunk = self.args
        coarse, fine = self.models
        for p in self.params:
            p.grad = None
        if self.sampler is not None:
            self.sampler.draw()                   # fills self.pixels / self.target (the sampler's buffers)
        poses = self.learned_poses()
        rays_o, rays_d = get_rays_indexed(H, W, K, poses, self.pixels, self.pose_index)
        rgb, disp, acc, extras = self.renderer.render_from_rays(H, W, K, chunk, torch.stack([rays_o, rays_d], 0), coarse, fine,
                                                                retraw=True)
        loss = img2mse(rgb, self.target)
        self.psnr = -10. * torch.log(loss.detach()) / math.log(10.)
        if 'rgb0' in extras:
            loss = loss + img2mse(extras['rgb0'], self.target)
        loss.backward()
        self.optimizer.step()
        self.loss = loss.detach()
        with torch.no_grad():
            self.poses = self.learned_poses()

    def __call__(self, pixels=None, pose_index=None, target=None):
        H, W = self.args[0], self.args[1]
        given = [a is not None for a in (pixels, pose_index, target)]
        if self.sampler is not None:
            if any(given):
                raise _lib.NerfAmdError("this step draws its own pixels (sampler=...): call step() without arguments")
        else:
            if not all(given):
                raise _lib.NerfAmdError("step(pixels, pose_index, target): a step built without a sampler needs all three")
            dev = self.pixels.device
            pix = pixels if (isinstance(pixels, torch.Tensor) and pixels.is_cuda) else _device_pixels(pixels, H, W, dev)
            idx = pose_index if (isinstance(pose_index, torch.Tensor) and pose_index.is_cuda) else \
                _host_pose_index(pose_index, self.pixels.shape[0], self.learned_poses.n_poses)
            self.pixels.copy_(pix, non_blocking=True)
            self.pose_index.copy_(idx, non_blocking=True)
            self.target.copy_(target, non_blocking=True)
        return self._replay()


def multistart_scores(losses, window=10):
    """The selection rule of multi-start pose estimation: losses [steps, B] -> (scores [B], best).  scores[b] is the mean of
    hypothesis b's last min(window, steps) losses (added in fp32, oldest first, then divided) with NaN counted as +inf; best =
    argmin(scores) (0-dim int64).  Runs where
    `losses` lives (no readback for a device tensor); a host array is taken as a CPU tensor."""
    losses = torch.as_tensor(losses)
    if losses.dim() != 2 or losses.shape[0] < 1 or losses.shape[1] < 1 or int(window) < 1:
        raise _lib.NerfAmdError("multistart_scores takes losses [steps >= 1, B >= 1] and window >= 1, got %s, %r" % (tuple(losses.shape), window))
    tail = losses[-min(int(window), losses.shape[0]):].float()
    tail = torch.where(torch.isnan(tail), torch.full_like(tail, float("inf")), tail)
    total = tail[0]
    for row in tail[1:]:                           # a DEFINED order (oldest step first, fp32): the scores can be restated exactly
        total = total + row
    scores = total / tail.shape[0]
    return scores, torch.argmin(scores)


def perturbed_start_poses(pose, n, rot_deg, trans, seed=0):
    """Hypotheses around a prior, for estimate_relative_pose_multistart: [n, 4, 4] float32 (host, numpy).  Entry 0 is `pose`
    itself; entry i > 0 is D_i @ pose with D_i a rotation by `rot_deg` degrees about a random unit axis (Rodrigues) and a
    translation of length `trans` in a random direction, both drawn from np.random.default_rng(seed): deterministic."""
    if isinstance(pose, torch.Tensor):
        pose = pose.detach().cpu().numpy()
    pose = np.asarray(pose, dtype=np.float64)
    if pose.shape != (4, 4) or int(n) < 1:
        raise _lib.NerfAmdError("perturbed_start_poses takes a [4, 4] pose and n >= 1, got %s, %r" % (pose.shape, n))
    rng = np.random.default_rng(seed)
    out = np.empty((int(n), 4, 4), dtype=np.float32)
    out[0] = pose
    a = np.deg2rad(float(rot_deg))
    for i in range(1, int(n)):
        axis, direction = rng.standard_normal(3), rng.standard_normal(3)
        axis, direction = axis / np.linalg.norm(axis), direction / np.linalg.norm(direction)
        Kx = np.array([[0., -axis[2], axis[1]], [axis[2], 0., -axis[0]], [-axis[1], axis[0], 0.]])
        D = np.eye(4)
        D[:3, :3] = np.eye(3) + np.sin(a) * Kx + (1. - np.cos(a)) * (Kx @ Kx)
        D[:3, 3] = float(trans) * direction
        out[i] = D @ pose
    return out


class PoseEstimate(tuple):
    """(pose, losses) of utils.estimate_relative_pose; `.step` is the CapturedPoseStep it ran (with .sampler, .cam_transf,
    .optimizer), for callers that want to go on or look inside."""

    def __new__(cls, pose, losses, step):
        self = super().__new__(cls, (pose, losses))
        self.step = step
        return self

    pose = property(lambda self: self[0])
    losses = property(lambda self: self[1])


def estimate_relative_pose(coarse_model, fine_model, renderer, sensor_image, start_pose, K, chunk, *, steps=300, batch_size=512,
                           lrate=0.01, strategy='interest_region', kernel_size=5, dil_iter=3, points=None, seed=0):
    """The pose-estimation demo's function (demo_est_rel_pose.py:26-98), sensor image in, pose out: the sampling region
    (PixelSampler), the se(3) module (CameraTransf), Adam over its seven numbers, and `steps` replays of one captured step
    with the demo's schedule, lr = lrate * 0.8 ** ((k + 1) / 100) set after step k.  A replay draws, renders, differentiates
    and updates on the device; the host writes the learning rate and nothing else, and nothing is read back inside the loop.

    Returns (pose, losses): the final [4, 4] camera-to-world (device) and the per-step losses [steps] (device).  The models must
    be frozen (requires_grad_(False)), as CapturedPoseStep demands; `points` are the caller's interest points (cv2 SIFT's, as
    in the demo) instead of the built-in detector's; `seed` fixes the draws.  (The returned tuple also carries `.step`, the
    captured step, for going on from there.)"""
    step, losses = _estimate_poses(CapturedPoseStep, CameraTransf, start_pose, chunk, (), coarse_model, fine_model, renderer,
                                   sensor_image, K, steps, batch_size, lrate, strategy, kernel_size, dil_iter, points, seed)
    return PoseEstimate(step.pose.clone(), losses, step)


def _estimate_poses(step_type, make_cam_transf, start, chunk, loss_shape, coarse_model, fine_model, renderer, sensor_image, K, steps,
                    batch_size, lrate, strategy, kernel_size, dil_iter, points, seed):
    """The loop of estimate_relative_pose and estimate_relative_pose_multistart: the sampler, the se(3) module that
    `make_cam_transf()` builds, Adam over it, one captured step of `step_type`, and `steps` replays with the demo's
    schedule.  Returns (step, losses [steps, *loss_shape])."""
    from . import optim
    H, W = int(sensor_image.shape[0]), int(sensor_image.shape[1])
    dev = next(coarse_model.parameters()).device
    sampler = PixelSampler(sensor_image, batch_size, strategy=strategy, points=points, kernel_size=kernel_size, dil_iter=dil_iter,
                           seed=seed, device=dev)
    cam_transf = make_cam_transf().to(dev)
    optimizer = optim.Adam(cam_transf.parameters(), lr=lrate, betas=(0.9, 0.999))
    step = step_type(renderer, H, W, K, chunk, coarse_model, fine_model, cam_transf, start, optimizer, batch_size, sampler=sampler)
    losses = torch.zeros(int(steps), *loss_shape, device=dev, dtype=torch.float32)
    for k in range(int(steps)):
        losses[k].copy_(step())
        for g in optimizer.param_groups:
            g['lr'] = lrate * (0.8 ** ((k + 1) / 100))
    return step, losses


class MultiPoseEstimate(PoseEstimate):
    """(pose, losses) of utils.estimate_relative_pose_multistart with `.poses` [B, 4, 4], `.scores` [B], `.best` (0-dim int64),
    all on the device, and `.step`, the CapturedMultiPoseStep it ran."""

    def __new__(cls, pose, losses, step, poses, scores, best):
        self = super().__new__(cls, pose, losses, step)
        self.poses, self.scores, self.best = poses, scores, best
        return self


def estimate_relative_pose_multistart(coarse_model, fine_model, renderer, sensor_image, start_poses, K, chunk, *, steps=300,
                                      batch_size=512, lrate=0.01, strategy='interest_region', kernel_size=5, dil_iter=3, points=None,
                                      seed=0, window=10):
    """estimate_relative_pose from B start poses [B, 4, 4] at once (utils.perturbed_start_poses makes them around a prior):
    one sampler, one CameraTransfBatch, one CapturedMultiPoseStep, the demo's learning-rate schedule.  Every hypothesis sees
    the same pixels at every step, so the per-step losses [steps, B] are comparable: scores[b] is the mean of hypothesis b's
    last min(window, steps) losses (NaN counts as +inf, multistart_scores) and best = argmin(scores), taken on the device --
    nothing is read back inside or after the loop.

    Returns (pose, losses) with pose = poses[best] (device [4, 4]) and losses [steps, B] (device); the tuple also carries
    .poses [B, 4, 4], .scores [B], .best (0-dim device int64) and .step (go on with step.cam_transfs.pose_module(int(best)))."""
    start_poses = torch.as_tensor(start_poses, dtype=torch.float32)
    if start_poses.dim() != 3 or tuple(start_poses.shape[1:]) != (4, 4):
        raise _lib.NerfAmdError("start_poses must be [B, 4, 4], got %s" % (tuple(start_poses.shape),))
    B = start_poses.shape[0]
    step, losses = _estimate_poses(CapturedMultiPoseStep, lambda: CameraTransfBatch(B), start_poses, max(int(chunk), B * int(batch_size)),
                                   (B,), coarse_model, fine_model, renderer, sensor_image, K, steps, batch_size, lrate, strategy,
                                   kernel_size, dil_iter, points, seed)
    scores, best = multistart_scores(losses, window)
    poses = step.poses.clone()
    return MultiPoseEstimate(poses.index_select(0, best.reshape(1))[0], losses, step, poses, scores, best)


def save_checkpoints(args, coarse_model, fine_model, optimizer, global_step, i):
    """<basedir>/<expname>/<i:06d>.tar with the reference's four keys (utils.py:444-456), so
    checkpoints move freely between this package and the reference."""
    path = os.path.join(args.basedir, args.expname, '{:06d}.tar'.format(i))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save({
        'global_step': global_step,
        'coarse_model_state_dict': coarse_model.state_dict(),
        'fine_model_state_dict': fine_model.state_dict() if fine_model is not None else None,
        'optimizer_state_dict': optimizer.state_dict(),
    }, path)
    print('Saved checkpoints at', path)
    return path


def load_checkpoint(coarse_model, fine_model, optimizer, args, b_load_ckpnt_as_trainable=False, checkpoint_index=None):
    """Reload the newest (or the indexed) *.tar of the experiment, or args.ft_path (utils.py:174-214).
    Returns the stored global_step (0 when nothing was loaded)."""
    if getattr(args, 'ft_path', None) is not None and args.ft_path != 'None':
        ckpts = [args.ft_path]
    else:
        folder = os.path.join(args.basedir, args.expname)
        ckpts = [os.path.join(folder, f) for f in sorted(os.listdir(folder)) if 'tar' in f] if os.path.isdir(folder) else []
    print('Found ckpts', ckpts)
    if not ckpts or getattr(args, 'no_reload', False):
        return 0
    path = ckpts[checkpoint_index] if checkpoint_index is not None else ckpts[-1]
    print('Reloading from', path)
    device = next(coarse_model.parameters()).device
    ckpt = torch.load(path, map_location=device)
    if optimizer is not None:
        optimizer.load_state_dict(ckpt['optimizer_state_dict'])
    coarse_model.load_state_dict(ckpt['coarse_model_state_dict'], strict=False)
    coarse_model.requires_grad_(b_load_ckpnt_as_trainable)
    if fine_model is not None:
        fine_model.load_state_dict(ckpt['fine_model_state_dict'])
        fine_model.requires_grad_(b_load_ckpnt_as_trainable)
    return ckpt['global_step']


# ---------------------------------------------------------------- datasets (utils.py:216-313)
def _scene_llff(args):
    """LLFF scene -> images, poses [N,3,4], render_poses, hwf, splits, (near, far)  (utils.py:220-252)."""
    from . import load_llff
    images, poses, bds, render_poses, i_test = load_llff.load_llff_data(
        args.datadir, args.factor, recenter=True, bd_factor=.75, spherify=args.spherify)
    hwf, poses = poses[0, :3, -1], poses[:, :3, :4]
    print('Loaded llff', images.shape, render_poses.shape, hwf, args.datadir)
    held_out = list(i_test) if isinstance(i_test, (list, tuple, np.ndarray)) else [i_test]
    if args.llffhold > 0:
        print('Auto LLFF holdout,', args.llffhold)
        held_out = np.arange(images.shape[0])[::args.llffhold]
    i_train = np.array([i for i in range(int(images.shape[0])) if i not in held_out])
    # world-space depth range from the scene bounds, or the unit NDC range
    near_far = (np.ndarray.min(bds) * .9, np.ndarray.max(bds) * 1.) if args.no_ndc else (0., 1.)
    print('NEAR FAR', *near_far)
    return images, poses, render_poses, hwf, (i_train, held_out, held_out), near_far


def _scene_blender(args):
    """NeRF-synthetic scene; RGBA is composited over white or the alpha dropped  (utils.py:254-266)."""
    from . import load_blender
    images, poses, render_poses, hwf, i_split, near, far = load_blender.load_blender_data(
        args.datadir, args.half_res, args.testskip)
    print('Loaded blender', images.shape, render_poses.shape, hwf, args.datadir)
    rgb, alpha = images[..., :3], images[..., -1:]
    images = rgb * alpha + (1. - alpha) if args.white_bkgd else rgb
    return images, poses, render_poses, hwf, tuple(i_split), (near, far)


_SCENE_READERS = {'llff': _scene_llff, 'blender': _scene_blender}


def load_datasets(args):
    """Scene on disk -> (images, poses, render_poses, [H, W, focal], (i_train, i_val, i_test), K,
    {'near', 'far'}) for dataset_type 'blender' and 'llff' (utils.py:216-313).  The LINEMOD and
    deepvoxels loaders of the reference are not part of this build."""
    reader = _SCENE_READERS.get(args.dataset_type)
    if reader is None:
        raise NotImplementedError("dataset_type %r: this build reads %s scenes" % (args.dataset_type, sorted(_SCENE_READERS)))
    images, poses, render_poses, hwf, (i_train, i_val, i_test), (near, far) = reader(args)
    H, W, focal = int(hwf[0]), int(hwf[1]), hwf[2]
    K = np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])
    if getattr(args, 'render_test', False):
        render_poses = np.array(poses[i_test])
    return images, poses, render_poses, [H, W, focal], (i_train, i_val, i_test), K, {'near': near, 'far': far}


# ---------------------------------------------------------------- training ray batches (utils.py:360-442)
def batch_training_data(args, poses, hwf, K, images, i_train):
    """Device-resident version of utils.py:360-392: with ray batching (not args.no_batching) the
    rays of every training image are generated on the GPU (make_rays kernel, no host meshgrid),
    joined with their pixels into rays_rgb [N_train*H*W, 3, 3] = (origin, direction, colour) and
    shuffled there.  Returns the reference's tuple."""
    H, W = int(hwf[0]), int(hwf[1])
    device = _default_device()
    images = torch.as_tensor(np.asarray(images), dtype=torch.float32, device=device) if not isinstance(images, torch.Tensor) \
        else images.to(device).float()
    poses = torch.as_tensor(np.asarray(poses), dtype=torch.float32, device=device) if not isinstance(poses, torch.Tensor) \
        else poses.to(device).float()
    use_batching = not args.no_batching
    if not use_batching:
        return images, poses, torch.empty(0, device=device), use_batching, args.N_rand, None
    blocks = []
    for i in i_train:
        b = make_ray_batch(H, W, K, poses[i, :3, :4], 0.0, 1.0, False, False, device=device)     # [H*W, 8]
        blocks.append(torch.stack([b[:, 0:3], b[:, 3:6], images[i].reshape(-1, 3)[:, :3]], 1))  # [H*W, 3, 3]
    rays_rgb = torch.cat(blocks, 0)
    rays_rgb = rays_rgb[torch.randperm(rays_rgb.shape[0], device=device)]
    return images, poses, rays_rgb, use_batching, args.N_rand, 0


def sample_random_ray_batch(args, images, poses, rays_rgb, N_rand, use_batching, i_batch, i_train, hwf, K, start, i):
    """One training batch (utils.py:394-442): the next N_rand rows of the shuffled ray bank
    (reshuffled on the device after an epoch), or N_rand random pixels of one random training
    image, centre-cropped during the first args.precrop_iters iterations.
    Returns batch_rays [2, N_rand, 3], target_s [N_rand, 3], rays_rgb, i_batch."""
    H, W = int(hwf[0]), int(hwf[1])
    if use_batching:
        batch = rays_rgb[i_batch:i_batch + N_rand].transpose(0, 1)
        batch_rays, target_s = batch[:2], batch[2]
        i_batch += N_rand
        if i_batch >= rays_rgb.shape[0]:
            print("Shuffle data after an epoch!")
            rays_rgb = rays_rgb[torch.randperm(rays_rgb.shape[0], device=rays_rgb.device)]
            i_batch = 0
        return batch_rays, target_s, rays_rgb, i_batch
    img_i = int(np.random.choice(i_train))
    target = images[img_i]
    rays_o, rays_d = get_rays(H, W, K, poses[img_i, :3, :4])
    if i < getattr(args, 'precrop_iters', 0):
        dH, dW = int(H // 2 * args.precrop_frac), int(W // 2 * args.precrop_frac)
        ys = torch.arange(H // 2 - dH, H // 2 + dH, device=target.device)
        xs = torch.arange(W // 2 - dW, W // 2 + dW, device=target.device)
        if i == start:
            print(f"[Config] Center cropping of size {2*dH} x {2*dW} is enabled until iter {args.precrop_iters}")
    else:
        ys, xs = torch.arange(H, device=target.device), torch.arange(W, device=target.device)
    n = ys.numel() * xs.numel()
    if N_rand > n:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")    # np.random.choice's error
    sel = torch.randperm(n, device=target.device)[:N_rand]            # without replacement, as np.random.choice(replace=False)
    yy, xx = ys[sel // xs.numel()], xs[sel % xs.numel()]
    batch_rays = torch.stack([rays_o[yy, xx], rays_d[yy, xx]], 0)
    return batch_rays, target[yy, xx][:, :3], rays_rgb, i_batch
