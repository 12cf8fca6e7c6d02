"""Thin tensor-level wrappers over the C ABI: argument checking, pointer plumbing, launch on
the tensors' own GPU and torch's current HIP stream of that GPU.  Every function requires
CUDA(HIP) float32 tensors; there is no CPU path."""

import ctypes
import math
import numbers
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import c_f, c_i, c_i64, c_p


class _DevPtr(ctypes.c_void_p):
    """A device pointer that remembers which GPU it points into (``device`` is None for a
    null pointer)."""
    device = None


def _dev(t: Optional[torch.Tensor], dtype=torch.float32, name="tensor"):
    if t is None:
        return _DevPtr(0)
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (got %s); the HIP path has no CPU fallback"
                           % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    ptr = _DevPtr(t.data_ptr())
    ptr.device = t.device
    return ptr


def _want(who, name, t, shape, dtype=torch.float32):
    """The argument contract of a wrapper ("The argument contract"): ``t`` is a
    contiguous ``dtype`` tensor of ``shape`` (``None`` = any extent), else ``ValueError`` (``TypeError``
    for the dtype, as ``_dev`` raises it) naming the wrapper and the argument.  Reads the tensor's
    metadata only: no device memory, no synchronisation."""
    if isinstance(t, torch.Tensor) and t.dtype == dtype:
        # the good case first, on plain ints: this runs in every launch of the training step
        got = t.shape
        if len(got) == len(shape):
            for w, g in zip(shape, got):
                if w is not None and w != g:
                    break
            else:
                if t.is_contiguous():
                    return
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: %s must be a %s tensor, got %s" % (who, name, dtype, type(t).__name__))
    if t.dtype != dtype:
        raise TypeError("%s: %s must be %s, got %s" % (who, name, dtype, t.dtype))
    got = t.shape
    if len(got) != len(shape) or any(w is not None and w != g for w, g in zip(shape, got)):
        raise ValueError("%s: %s must be (%s), got %s"
                         % (who, name, ", ".join("*" if w is None else str(w) for w in shape),
                            tuple(got)))
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (who, name))


def _want_numel(who, name, t, numel, dtype=torch.float32, at_least=False):
    """``_want`` for a buffer the entry point takes as a flat extent: ``numel`` elements exactly
    (``at_least``: or more), whatever the shape."""
    if isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous():
        have = t.numel()
        if have == numel or (at_least and have > numel):
            return
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s: %s must be a %s tensor, got %s" % (who, name, dtype, type(t).__name__))
    if t.dtype != dtype:
        raise TypeError("%s: %s must be %s, got %s" % (who, name, dtype, t.dtype))
    if t.numel() != numel and not (at_least and t.numel() > numel):
        raise ValueError("%s: %s must hold %s%d elements, got %s = %d"
                         % (who, name, "at least " if at_least else "", numel, tuple(t.shape),
                            t.numel()))
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (who, name))


def _want_tensors(who, **named):
    """Every named argument is a tensor (the checks that follow read ``.shape`` and ``.dim()``)."""
    for name, t in named.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))


def _want_int(who, name, value, low, high=None):
    """An integer argument inside the bounds include/ffn_hip.h documents for it."""
    if type(value) is int and value >= low and (high is None or value <= high):
        return
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or value < low or (high is not None
                                                                         and value > high):
        raise ValueError("%s: %s must be an integer %s, got %r"
                         % (who, name, ">= %d" % low if high is None else "in %d .. %d" % (low, high),
                            value))


def _call(name, *args):
    """Launches entry point ``name`` on the GPU its tensor arguments live on: that GPU is made
    current for the call (the C ABI launches on the calling thread's current device) and the
    kernel goes onto torch's current stream OF THAT GPU, which is appended as the trailing
    ``stream`` argument.  Tensors on different GPUs in one call are an error."""
    device = None
    for a in args:
        d = getattr(a, "device", None)
        if d is None:
            continue
        if device is None:
            device = d
        elif d != device:
            raise RuntimeError("%s: tensor arguments live on different devices (%s and %s)"
                               % (name, device, d))
    if device is None:
        raise RuntimeError("%s: no device tensor among the arguments" % name)
    stream = c_p(torch.cuda.current_stream(device).cuda_stream)
    if device.index == torch.cuda.current_device():
        return _lib.call(name, *args, stream)
    with torch.cuda.device(device):
        return _lib.call(name, *args, stream)


def _host3(values):
    arr = (ctypes.c_float * 3)(*[float(v) for v in values])
    return arr


# --------------------------------------------------------------------------------- rays
def raygen_nearfar(unproj: torch.Tensor, cam_pos: torch.Tensor, width: int, height: int,
                   box_lo, box_hi, points: Optional[torch.Tensor] = None):
    """K1.  unproj (C,4,4), cam_pos (C,3) on the GPU -> starts, directions, near_far, valid.
    ``points`` (W*H,2) float32 overrides the integer pixel grid."""
    who = "raygen_nearfar"
    if not isinstance(unproj, torch.Tensor) or unproj.dim() not in (2, 3):
        raise ValueError("%s: unproj must be a (C,4,4) or (C,16) tensor" % who)
    cams = unproj.shape[0]
    _want_numel(who, "unproj", unproj, 16 * cams)
    _want(who, "cam_pos", cam_pos, (cams, 3))
    _want_int(who, "width", width, 1)
    _want_int(who, "height", height, 1)
    if points is not None:
        _want(who, "points", points, (width * height, 2))
    total = cams * width * height
    dev = unproj.device
    starts = torch.empty((total, 3), dtype=torch.float32, device=dev)
    dirs = torch.empty((total, 3), dtype=torch.float32, device=dev)
    near_far = torch.empty((2, total), dtype=torch.float32, device=dev)
    valid = torch.empty((total,), dtype=torch.uint8, device=dev)
    _call("ffn_raygen_nearfar", _dev(unproj, name="unproj"), _dev(cam_pos, name="cam_pos"),
              _dev(points, name="points"), c_i(cams), c_i(width), c_i(height), _host3(box_lo), _host3(box_hi), _dev(starts),
              _dev(dirs), _dev(near_far), _dev(valid, torch.uint8))
    return starts, dirs, near_far, valid


def sample_t(near_far: torch.Tensor, ray_index: torch.Tensor, count: int, unit: torch.Tensor,
             noise: Optional[torch.Tensor], anneal: Optional[float],
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K2a.  Returns (R, stride) t-values; the first `count` columns are filled."""
    who = "sample_t"
    _want(who, "near_far", near_far, (2, None))
    _want(who, "ray_index", ray_index, (None,), torch.int64)
    rays = ray_index.shape[0]
    _want_int(who, "count", count, 1)
    _want(who, "unit", unit, (count,))
    if noise is not None:
        _want(who, "noise", noise, (rays, count))
    if out is not None:
        _want(who, "out", out, (rays, None))
        if out.shape[1] < count:
            raise ValueError("%s: out must be (%d, >= %d), got %s"
                             % (who, rays, count, tuple(out.shape)))
    if out is None:
        out = torch.empty((rays, count), dtype=torch.float32, device=near_far.device)
    _call("ffn_sample_t", _dev(near_far), c_i64(near_far.shape[1]),
              _dev(ray_index, torch.int64, "ray_index"), c_i(rays), c_i(count), _dev(unit),
              _dev(noise), c_f(-1.0 if anneal is None else float(anneal)), _dev(out),
              c_i(out.shape[1]))
    return out


def materialise_samples(starts, directions, ray_index, t_values, want_views=True):
    """K2b.  positions (R,S,3) [and view_directions (R,S,3)]."""
    who = "materialise_samples"
    _want(who, "t_values", t_values, (None, None))
    rays, count = t_values.shape
    _want(who, "ray_index", ray_index, (rays,), torch.int64)
    _want(who, "starts", starts, (None, 3))
    _want(who, "directions", directions, (starts.shape[0], 3))
    pos = torch.empty((rays, count, 3), dtype=torch.float32, device=t_values.device)
    views = torch.empty_like(pos) if want_views else None
    _call("ffn_materialise_samples", _dev(starts), _dev(directions),
              _dev(ray_index, torch.int64), _dev(t_values), c_i(rays), c_i(count), _dev(pos),
              _dev(views))
    return pos, views


def sample_materialise(near_far, starts, directions, ray_index, count, unit, noise, anneal, want_views=True):
    """K2a + K2b in one launch: t (R,count), positions (R,count,3) [, view_directions]."""
    who = "sample_materialise"
    try:            # every launch of a training step comes through here: the good case on plain ints
        good = (type(count) is int and count >= 1 and near_far.dim() == 2 and near_far.shape[0] == 2
                and starts.dim() == 2 and starts.shape[1] == 3 and directions.shape == starts.shape
                and ray_index.dim() == 1 and unit.shape == (count,)
                and (noise is None or noise.shape == (ray_index.shape[0], count)))
    except (AttributeError, TypeError):
        good = False
    if not good:    # (dtype and contiguity are ``_dev``'s, before the one launch)
        _want(who, "near_far", near_far, (2, None))
        _want(who, "starts", starts, (None, 3))
        _want(who, "directions", directions, (starts.shape[0], 3))
        _want(who, "ray_index", ray_index, (None,), torch.int64)
        _want_int(who, "count", count, 1)
        _want(who, "unit", unit, (count,))
        if noise is not None:
            _want(who, "noise", noise, (ray_index.shape[0], count))
    rays = ray_index.shape[0]
    t = torch.empty((rays, count), dtype=torch.float32, device=near_far.device)
    pos = torch.empty((rays, count, 3), dtype=torch.float32, device=near_far.device)
    views = torch.empty_like(pos) if want_views else None
    _call("ffn_sample_materialise", _dev(near_far), c_i64(near_far.shape[1]), _dev(starts), _dev(directions),
          _dev(ray_index, torch.int64, "ray_index"), c_i(rays), c_i(count), _dev(unit), _dev(noise),
          c_f(-1.0 if anneal is None else float(anneal)), _dev(t), _dev(pos), _dev(views))
    return t, pos, views


def cdf_build(t_probe: torch.Tensor, opacity: torch.Tensor) -> torch.Tensor:
    """K2c.  (P,n),(P,n) -> (P,n-1)."""
    _want("cdf_build", "t_probe", t_probe, (None, None))
    rays, n = t_probe.shape
    _want_int("cdf_build", "t_probe.shape[1]", n, 1)
    _want("cdf_build", "opacity", opacity, (rays, n))
    cdf = torch.empty((rays, n - 1), dtype=torch.float32, device=t_probe.device)
    _call("ffn_cdf_build", _dev(t_probe), _dev(opacity), c_i64(rays), c_i(n), _dev(cdf))
    return cdf


def cdf_build_logits(t_probe: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
    """K2c on raw coarse-model outputs: (P,n), (P*n,4) -> (P,n-1); softplus inside."""
    _want("cdf_build_logits", "t_probe", t_probe, (None, None))
    rays, n = t_probe.shape
    _want_int("cdf_build_logits", "t_probe.shape[1]", n, 1)
    _want_numel("cdf_build_logits", "logits", logits, rays * n * 4)
    cdf = torch.empty((rays, n - 1), dtype=torch.float32, device=t_probe.device)
    _call("ffn_cdf_build_logits", _dev(t_probe), _dev(logits), c_i64(rays), c_i(n), _dev(cdf))
    return cdf


def focus_sample_merge(near_far, cdfs, ray_index, u, unit_focus, t_io, n_focus, rows_local=False):
    """K2d.  In-place on t_io (R,S).  ``rows_local``: cdfs holds one row per batch ray."""
    who = "focus_sample_merge"
    _want(who, "t_io", t_io, (None, None))
    rays, count = t_io.shape
    _want_int(who, "t_io.shape[1]", count, 1, 256)
    _want_int(who, "n_focus", n_focus, 1, count)
    _want(who, "near_far", near_far, (2, None))
    _want(who, "cdfs", cdfs, (rays if rows_local else None, n_focus - 1))
    if not rows_local and cdfs.shape[0] < near_far.shape[1]:
        raise ValueError("%s: cdfs holds %d rows, fewer than the %d rays of near_far that index it"
                         % (who, cdfs.shape[0], near_far.shape[1]))
    _want(who, "ray_index", ray_index, (rays,), torch.int64)
    _want(who, "u", u, (rays, n_focus))
    _want(who, "unit_focus", unit_focus, (n_focus,))
    _call("ffn_focus_sample_merge_rows" if rows_local else "ffn_focus_sample_merge", _dev(near_far), c_i64(near_far.shape[1]), _dev(cdfs),
              _dev(ray_index, torch.int64), _dev(u), _dev(unit_focus), c_i(rays), c_i(count),
              c_i(n_focus), _dev(t_io))
    return t_io


def to_image(colors: torch.Tensor, pixel_index: torch.Tensor, width: int, height: int):
    """K8.  (n,3) colours + (n,) pixel ids -> (H,W,3) uint8 on the GPU: the byte of a colour
    ``c`` is ``float32(c) * 255`` truncated, unlisted pixels are 0."""
    for name, t in (("colors", colors), ("pixel_index", pixel_index)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("to_image: %s must be a tensor, got %s" % (name, type(t).__name__))
    if colors.dim() != 2 or colors.shape[1] != 3:
        raise ValueError("to_image: colors must be (n, 3), got %s" % (tuple(colors.shape),))
    if pixel_index.numel() != colors.shape[0]:
        raise ValueError("to_image: %d pixel ids for %d colours" % (pixel_index.numel(), colors.shape[0]))
    if width <= 0 or height <= 0:
        raise ValueError("to_image: width and height must be positive, got %d x %d" % (width, height))
    if colors.shape[0] > width * height:
        raise ValueError("to_image: %d colours for a frame of %d x %d pixels" % (colors.shape[0], width, height))
    if pixel_index.device != colors.device:
        raise RuntimeError("to_image: tensor arguments live on different devices (%s and %s)"
                           % (colors.device, pixel_index.device))
    img =torch.empty((height, width, 3), dtype=torch.uint8, device=colors.device)
    _call("ffn_to_image", _dev(colors), _dev(pixel_index, torch.int64),
              c_i64(colors.shape[0]), c_i(width), c_i(height), _dev(img, torch.uint8))
    return img


def ycrcb_to_rgb_u8(image: torch.Tensor) -> torch.Tensor:
    """K8b.  (H,W,3) uint8 YCrCb frame -> RGB, in place (OpenCV's 8-bit COLOR_YCrCb2RGB)."""
    who = "ycrcb_to_rgb_u8"
    if not isinstance(image, torch.Tensor) or image.dim() < 1 or image.shape[-1] != 3:
        raise ValueError("%s: image must be a (..., 3) torch.uint8 frame, got %s"
                         % (who, tuple(image.shape) if isinstance(image, torch.Tensor)
                            else type(image).__name__))
    _want_numel(who, "image", image, image.numel(), torch.uint8)
    _call("ffn_ycrcb_to_rgb_u8", _dev(image, torch.uint8, "image"), c_i64(image.numel() // 3))
    return image


# --------------------------------------------------------------------------------- encode
def fourier_encode(x: torch.Tensor, b: Optional[torch.Tensor], a: Optional[torch.Tensor],
                   scale: float, include_input: bool) -> torch.Tensor:
    """K3.  (N,3) -> (N, 2F[+3]) with the cos block first; b (3,F) or None, a (F) or None."""
    if not isinstance(x, torch.Tensor):
        raise ValueError("fourier_encode: x must be a tensor, got %s" % type(x).__name__)
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("fourier_encode: x must be (N, 3), got %s" % (tuple(x.shape),))
    if b is not None and (b.dim() != 2 or b.shape[0] != 3):
        raise ValueError("fourier_encode: b must be (3, F), got %s" % (tuple(b.shape),))
    n = x.shape[0]
    freq = 0 if b is None else b.shape[1]
    if a is not None and a.numel() != freq:
        raise ValueError("fourier_encode: a has %d values for %d frequencies" % (a.numel(), freq))
    for name, t in (("b", b), ("a", a)):
        if t is not None and t.device != x.device:
            raise RuntimeError("fourier_encode: tensor arguments live on different devices (x on %s, %s on %s)"
                               % (x.device, name, t.device))
    width = 2 * freq + (3 if (include_input or freq == 0) else 0)
    out = torch.empty((n, width), dtype=torch.float32, device=x.device)
    _call("ffn_fourier_encode", _dev(x), c_i64(n), _dev(b), _dev(a), c_i(freq),
              c_f(scale), c_i(1 if include_input else 0), _dev(out))
    return out


# --------------------------------------------------------------------------------- composite
def composite_fwd(logits: torch.Tensor, t: torch.Tensor, include_depth: bool,
                  nan_flag: Optional[torch.Tensor] = None):
    """K5.  logits (R,S,4), t (R,S) -> color (R,3), alpha (R), depth (R)|None."""
    _want("composite_fwd", "t", t, (None, None))
    rays, count = t.shape
    _want_numel("composite_fwd", "logits", logits, rays * count * 4)
    if nan_flag is not None:
        _want_numel("composite_fwd", "nan_flag", nan_flag, 1, torch.int32)
    dev = t.device
    color = torch.empty((rays, 3), dtype=torch.float32, device=dev)
    alpha = torch.empty((rays,), dtype=torch.float32, device=dev)
    depth = torch.empty((rays,), dtype=torch.float32, device=dev) if include_depth else None
    _call("ffn_composite_fwd", _dev(logits), _dev(t), c_i(rays), c_i(count), _dev(color),
              _dev(alpha), _dev(depth), _dev(nan_flag, torch.int32))
    return color, alpha, depth


def blend_weights(t: torch.Tensor, sigma: torch.Tensor) -> torch.Tensor:
    """K5w.  utils.calculate_blend_weights: (R,S),(R,S) -> (R,S)."""
    _want("blend_weights", "t", t, (None, None))
    rays, count = t.shape
    _want("blend_weights", "sigma", sigma, (rays, count))
    out = torch.empty_like(t)
    _call("ffn_blend_weights", _dev(t), _dev(sigma), c_i(rays), c_i(count), _dev(out))
    return out


def blend_weights_bwd(t: torch.Tensor, sigma: torch.Tensor, d_weights: torch.Tensor,
                      want_dt: bool = False):
    """K5w backward.  Returns (d_sigma (R,S), d_t (R,S) | None)."""
    who = "blend_weights_bwd"
    _want(who, "t", t, (None, None))
    rays, count = t.shape
    _want(who, "sigma", sigma, (rays, count))
    _want(who, "d_weights", d_weights, (rays, count))
    d_sigma = torch.empty_like(t)
    d_t = torch.empty_like(t) if want_dt else None
    _call("ffn_blend_weights_bwd", _dev(t), _dev(sigma), _dev(d_weights), c_i(rays), c_i(count),
          _dev(d_sigma), _dev(d_t))
    return d_sigma, d_t


def composite_bwd(logits, t, d_color, d_alpha) -> torch.Tensor:
    """K5b.  d(logits) (R,S,4)."""
    who = "composite_bwd"
    _want(who, "t", t, (None, None))
    rays, count = t.shape
    _want_numel(who, "logits", logits, rays * count * 4)
    _want(who, "d_color", d_color, (rays, 3))
    _want(who, "d_alpha", d_alpha, (rays,))
    d_logits = torch.empty((rays, count, 4), dtype=torch.float32, device=t.device)
    _call("ffn_composite_bwd", _dev(logits), _dev(t), _dev(d_color), _dev(d_alpha),
              c_i(rays), c_i(count), _dev(d_logits))
    return d_logits


def mse_loss(color, alpha, gt_colors, gt_alphas, ray_index, color_scale, alpha_scale,
             want_grad=True, sums_out=None):
    """K6.  Returns (sums (2,), d_color, d_alpha); ``sums_out`` (2 floats) receives the sums
    in place of a fresh tensor."""
    who = "mse_loss"
    _want(who, "color", color, (None, 3))
    rays = color.shape[0]
    _want(who, "alpha", alpha, (rays,))
    _want(who, "gt_colors", gt_colors, (None, 3))
    if gt_alphas is not None:
        _want(who, "gt_alphas", gt_alphas, (gt_colors.shape[0],))
    _want(who, "ray_index", ray_index, (rays,), torch.int64)
    if sums_out is not None:
        _want_numel(who, "sums_out", sums_out, 2)
    dev = color.device
    sums = sums_out if sums_out is not None else torch.empty((2,), dtype=torch.float32, device=dev)
    scratch = torch.empty((2 * ((rays + 255) // 256),), dtype=torch.float32, device=dev)
    d_color = torch.empty_like(color) if want_grad else None
    d_alpha = torch.empty_like(alpha) if want_grad else None
    _call("ffn_mse_loss", _dev(color), _dev(alpha), _dev(gt_colors), _dev(gt_alphas),
              _dev(ray_index, torch.int64), c_i(rays), c_f(color_scale), c_f(alpha_scale),
              _dev(sums), _dev(d_color), _dev(d_alpha), _dev(scratch))
    return sums, d_color, d_alpha


def composite_train(logits, t, gt_colors, gt_alphas, ray_index, color_scale, alpha_scale,
                    nan_flag: Optional[torch.Tensor] = None):
    """K5t: K5 + K6 + K5b of one training batch in one launch.  logits (R,S,4), t (R,S) ->
    (d_logits (R,S,4), partials (blocks,2)): d_logits bit-identical to ``composite_fwd`` ->
    ``mse_loss`` -> ``composite_bwd``; the loss sums per workgroup go to ``loss_from_partials``."""
    who = "composite_train"
    try:            # every launch of a training step comes through here: the good case on plain ints
        rays, count = t.shape
        good = (logits.numel() == rays * count * 4 and gt_colors.dim() == 2
                and gt_colors.shape[1] == 3 and ray_index.shape == (rays,)
                and (gt_alphas is None or gt_alphas.shape == (gt_colors.shape[0],))
                and (nan_flag is None or nan_flag.numel() == 1))
    except (AttributeError, TypeError, ValueError):
        good = False
    if not good:    # (dtype and contiguity are ``_dev``'s, before the one launch)
        _want(who, "t", t, (None, None))
        rays, count = t.shape
        _want_numel(who, "logits", logits, rays * count * 4)
        _want(who, "gt_colors", gt_colors, (None, 3))
        if gt_alphas is not None:
            _want(who, "gt_alphas", gt_alphas, (gt_colors.shape[0],))
        _want(who, "ray_index", ray_index, (rays,), torch.int64)
        if nan_flag is not None:
            _want_numel(who, "nan_flag", nan_flag, 1, torch.int32)
    blocks = int(_lib.load().ffn_composite_train_blocks(c_i(rays)))
    d_logits = torch.empty((rays, count, 4), dtype=torch.float32, device=t.device)
    partials = torch.empty((blocks, 2), dtype=torch.float32, device=t.device)
    _call("ffn_composite_train", _dev(logits), _dev(t), c_i(rays), c_i(count), _dev(gt_colors),
          _dev(gt_alphas), _dev(ray_index, torch.int64), c_f(color_scale), c_f(alpha_scale),
          _dev(d_logits), _dev(partials), _dev(nan_flag, torch.int32))
    return d_logits, partials


def loss_from_partials(partials: torch.Tensor, rays: int, alpha_weight: float,
                       sums_out: Optional[torch.Tensor] = None, want_loss: bool = True):
    """Fixed-order sum of K5t's per-workgroup pairs: into ``sums_out`` (2 floats, for the
    data-parallel all-reduce) and / or the scalar loss (a fresh device scalar)."""
    _want("loss_from_partials", "partials", partials, (None, 2))
    if sums_out is not None:
        _want_numel("loss_from_partials", "sums_out", sums_out, 2)
    loss = torch.empty((), dtype=torch.float32, device=partials.device) if want_loss else None
    _call("ffn_loss_from_partials", _dev(partials), c_i(partials.shape[0]), c_f(3.0 * rays),
          c_f(float(rays)), c_f(alpha_weight), _dev(sums_out), _dev(loss))
    return loss


def loss_value(sums: torch.Tensor, rays: int, alpha_weight: float) -> torch.Tensor:
    """sums[0] / (3 rays) + alpha_weight * sums[1] / rays as a fresh device scalar (one launch)."""
    _want_numel("loss_value", "sums", sums, 2)
    out = torch.empty((), dtype=torch.float32, device=sums.device)
    _call("ffn_loss_value", _dev(sums), c_f(3.0 * rays), c_f(float(rays)), c_f(alpha_weight), _dev(out))
    return out


# --------------------------------------------------------------------------------- regression
def regression_blocks(n: int) -> int:
    """Workgroups (= partial sums) of K11 for ``n`` pixels."""
    return int(_lib.load().ffn_regression_blocks(c_i64(n)))


def _regression_want(who, logits, target, c, d_logits, partials, partials_needed=True):
    """What K11 and K11b share: logits (n,4), target (n,c) with 1 <= c <= 4 (``target`` None: ``c``
    from the caller), d_logits (n,4) where there is one, ``regression_blocks(n)`` partials."""
    if c is not None:
        _want_int(who, "c", c, 1, 4)
    if target is not None:
        _want(who, "target", target, (None, c))
        n, c = target.shape
        _want_int(who, "target.shape[1]", c, 1, 4)
        _want(who, "logits", logits, (n, 4))
    else:
        _want(who, "logits", logits, (None, 4))
        n = logits.shape[0]
    if d_logits is not None:
        _want(who, "d_logits", d_logits, (n, 4))
    if partials is not None:
        _want_numel(who, "partials", partials, regression_blocks(n) if n > 0 else 0, at_least=True)
    elif partials_needed:
        raise ValueError("%s: partials must be a torch.float32 tensor, got NoneType" % who)
    return n, c


def regression_train(logits: torch.Tensor, target: torch.Tensor, d_logits: torch.Tensor,
                     partials: torch.Tensor):
    """K11 training: logits (n,4), target (n,c) -> d_logits (n,4) of 0.5 * mean((sigmoid - y)^2)
    (columns >= c exactly 0) and one sum of squares per workgroup in ``partials``."""
    _want("regression_train", "target", target, (None, None))
    _want("regression_train", "d_logits", d_logits, (None, 4))
    _regression_want("regression_train", logits, target, None, d_logits, partials)
    n, c = target.shape
    _call("ffn_regression_train", _dev(logits, name="logits"), _dev(target, name="target"),
          c_i64(n), c_i(c), c_f(1.0 / (n * c)), _dev(d_logits, name="d_logits"),
          _dev(partials, name="partials"))


def regression_eval(logits: torch.Tensor, target: Optional[torch.Tensor], c: int,
                    partials: Optional[torch.Tensor], image: Optional[torch.Tensor] = None):
    """K11 validation: sums of (sigmoid - y)^2 per workgroup into ``partials`` and / or the
    (sigmoid * 255) u8 pixels (n,c) into ``image``."""
    who = "regression_eval"
    if partials is not None and target is None:
        raise ValueError("%s: partials need a target to compare with" % who)
    n, c = _regression_want(who, logits, target, c, None, partials, partials_needed=False)
    if image is not None:
        _want_numel(who, "image", image, n * c, torch.uint8)
    _call("ffn_regression_eval", _dev(logits, name="logits"), _dev(target, name="target"),
          c_i64(n), c_i(c), _dev(partials, name="partials"), _dev(image, torch.uint8, "image"))


def _regression_loss_want(who, partials, sse_out, loss_out):
    _want(who, "partials", partials, (None,))
    for name, t in (("sse_out", sse_out), ("loss_out", loss_out)):
        if t is not None:
            _want_numel(who, name, t, 1)


def regression_loss(partials: torch.Tensor, count: int, sse_out: Optional[torch.Tensor] = None,
                    loss_out: Optional[torch.Tensor] = None):
    """Fixed-order sum of K11's partials: sse into ``sse_out``, 0.5 * sse / count into ``loss_out``."""
    _regression_loss_want("regression_loss", partials, sse_out, loss_out)
    _call("ffn_regression_loss", _dev(partials), c_i(partials.shape[0]), c_f(float(count)),
          _dev(sse_out), _dev(loss_out))


def inv_count(count: int) -> float:
    """fl32(1 / count), divided in float32 as ATen's mean backward does (not rounded from a
    float64 quotient)."""
    return float(np.float32(1.0) / np.float32(count))


def regression_mse_train(logits: torch.Tensor, target: torch.Tensor, d_logits: torch.Tensor,
                         partials: torch.Tensor):
    """K11b training: logits (n,4), target (n,c) -> d_logits (n,4) of mean((z - y)^2) (columns
    >= c exactly 0) and one sum of squares per workgroup in ``partials``."""
    _want("regression_mse_train", "target", target, (None, None))
    _want("regression_mse_train", "d_logits", d_logits, (None, 4))
    _regression_want("regression_mse_train", logits, target, None, d_logits, partials)
    n, c = target.shape
    _call("ffn_regression_mse_train", _dev(logits, name="logits"), _dev(target, name="target"),
          c_i64(n), c_i(c), c_f(inv_count(n * c)), _dev(d_logits, name="d_logits"),
          _dev(partials, name="partials"))


def regression_mse_eval(logits: torch.Tensor, target: torch.Tensor, partials: torch.Tensor):
    """K11b validation: sums of (z - y)^2 per workgroup into ``partials``."""
    _want("regression_mse_eval", "target", target, (None, None))
    _regression_want("regression_mse_eval", logits, target, None, None, partials)
    n, c = target.shape
    _call("ffn_regression_mse_eval", _dev(logits, name="logits"), _dev(target, name="target"),
          c_i64(n), c_i(c), _dev(partials, name="partials"))


def regression_mse_loss(partials: torch.Tensor, count: int, sse_out: Optional[torch.Tensor] = None,
                        loss_out: Optional[torch.Tensor] = None):
    """Fixed-order sum of K11b's partials: sse into ``sse_out``, sse / count into ``loss_out``."""
    _regression_loss_want("regression_mse_loss", partials, sse_out, loss_out)
    _call("ffn_regression_mse_loss", _dev(partials), c_i(partials.shape[0]), c_f(float(count)),
          _dev(sse_out), _dev(loss_out))


# --------------------------------------------------------------------------------- optimiser
def clip_adam(params, grads, exp_avg, exp_avg_sq, step: int, lr: float, weight_decay=0.0,
              clip_value=0.1, max_norm=0.1, beta1=0.9, beta2=0.999, eps=1e-8,
              scratch=None, norm_out=None):
    """K7 on flat fp32 buffers; `step` is the 1-based update count."""
    who = "clip_adam"
    if not isinstance(params, torch.Tensor):
        raise ValueError("%s: params must be a torch.float32 tensor, got %s"
                         % (who, type(params).__name__))
    n = params.numel()
    _want_numel(who, "params", params, n)
    _want_numel(who, "grads", grads, n)
    _want_numel(who, "exp_avg", exp_avg, n)
    _want_numel(who, "exp_avg_sq", exp_avg_sq, n)
    _want_int(who, "step", step, 1)
    if scratch is not None:
        _want_numel(who, "scratch", scratch, (n + 1023) // 1024, at_least=True)
    if norm_out is not None:
        _want_numel(who, "norm_out", norm_out, 1)
    if scratch is None:
        scratch = torch.empty(((n + 1023) // 1024,), dtype=torch.float32, device=params.device)
    step_size = lr / (1.0 - beta1 ** step)
    inv_sqrt_bc2 = 1.0 / math.sqrt(1.0 - beta2 ** step)
    _call("ffn_clip_adam", _dev(params), _dev(grads), _dev(exp_avg), _dev(exp_avg_sq),
              c_i64(n), c_f(clip_value), c_f(max_norm), c_f(step_size), c_f(inv_sqrt_bc2),
              c_f(beta1), c_f(beta2), c_f(eps), c_f(weight_decay), _dev(scratch),
              _dev(norm_out))


# --------------------------------------------------------------------------------- occupancy
def occupancy_build(logits: torch.Tensor, resolution: int, sigma_threshold: float,
                    dilate: bool) -> torch.Tensor:
    """K9a/b.  logits (G^3,4) at the cell centres -> bit mask (ceil(G^3/32),) int32."""
    _want_int("occupancy_build", "resolution", resolution, 1)
    _want_numel("occupancy_build", "logits", logits, 4 * resolution ** 3)
    words = (resolution ** 3 + 31) // 32
    bits = torch.empty((words,), dtype=torch.int32, device=logits.device)
    scratch = torch.empty_like(bits) if dilate else None
    _call("ffn_occupancy_build", _dev(logits), c_i(resolution), c_f(sigma_threshold),
              c_i(1 if dilate else 0), _dev(scratch, torch.int32), _dev(bits, torch.int32))
    return bits


def occupancy_compact(positions: torch.Tensor, views: Optional[torch.Tensor], box_min, box_size,
                      resolution: int, bits: torch.Tensor):
    """K9c-e.  (N,3) samples -> packed positions / views of the samples in occupied cells and
    their int32 source index.  One device-to-host sync (the packed count sizes the outputs)."""
    who = "occupancy_compact"
    _want(who, "positions", positions, (None, 3))
    if views is not None:
        _want(who, "views", views, (positions.shape[0], 3))
    _want_int(who, "resolution", resolution, 1)
    _want_numel(who, "bits", bits, (resolution ** 3 + 31) // 32, torch.int32)
    n = positions.shape[0]
    dev = positions.device
    blocks = (n + 255) // 256
    offsets = torch.empty((blocks,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int64, device=dev)
    lo, size = _host3(box_min), _host3(box_size)
    _call("ffn_occupancy_count", _dev(positions), c_i64(n), lo, size, c_i(resolution),
              _dev(bits, torch.int32), _dev(offsets, torch.int32), _dev(total, torch.int64))
    m = int(total.item())
    out_pos = torch.empty((m, 3), dtype=torch.float32, device=dev)
    out_view = torch.empty((m, 3), dtype=torch.float32, device=dev) if views is not None else None
    index = torch.empty((m,), dtype=torch.int32, device=dev)
    if m > 0:
        _call("ffn_occupancy_compact", _dev(positions), _dev(views), c_i64(n), lo, size,
                  c_i(resolution), _dev(bits, torch.int32), _dev(offsets, torch.int32),
                  _dev(out_pos), _dev(out_view), _dev(index, torch.int32))
    return out_pos, out_view, index


def occupancy_from_octree_check(leaf_index, scale, center, box_min, box_size, resolution,
                                rows=None, stride=4, sigma_offset=3, sigma_threshold=None,
                                dilate=0, out=None) -> int:
    """The refusals of ``occupancy_from_octree``, none of which needs a device.  Tensors on any
    device.  -> the number of int32 words of the grid.  Raises ``ValueError`` naming the argument."""
    who = "occupancy_from_octree"
    resolution = int(resolution)
    if not 1 <= resolution <= 1024:
        raise ValueError("%s: resolution must lie in 1 .. 1024, got %d" % (who, resolution))
    if (not torch.is_tensor(leaf_index) or leaf_index.dtype != torch.int64 or leaf_index.dim() != 1
            or not 1 <= leaf_index.shape[0] < 1 << 31):
        raise ValueError("%s: leaf_index must be a (L,) int64 tensor of 1 .. 2^31 - 1 leaves" % who)
    scale = float(np.float32(scale))
    if not (math.isfinite(scale) and scale > 0):
        raise ValueError("%s: scale must be finite and positive, got %r" % (who, scale))
    for name, vec in (("center", center), ("box_min", box_min), ("box_size", box_size)):
        vec = [float(np.float32(v)) for v in vec]
        if len(vec) != 3 or not all(math.isfinite(v) for v in vec):
            raise ValueError("%s: %s must be three finite numbers, got %r" % (who, name, vec))
        if name == "box_size" and not all(v > 0 for v in vec):
            raise ValueError("%s: box_size must be positive, got %r" % (who, vec))
    if rows is None:
        if sigma_threshold is not None:
            raise ValueError("%s: sigma_threshold needs the leaves' density (rows); this tree has "
                             "none" % who)
    else:
        stride, sigma_offset = int(stride), int(sigma_offset)
        if stride < 1 or not 0 <= sigma_offset < stride:
            raise ValueError("%s: stride >= 1 and 0 <= sigma_offset < stride, got stride %d, "
                             "sigma_offset %d" % (who, stride, sigma_offset))
        if (not torch.is_tensor(rows) or rows.dtype != torch.float32
                or tuple(rows.shape) != (leaf_index.shape[0], stride)):
            raise ValueError("%s: rows must be (%d, %d) float32, got %s"
                             % (who, leaf_index.shape[0], stride,
                                tuple(rows.shape) if torch.is_tensor(rows) else type(rows).__name__))
    if sigma_threshold is not None and math.isnan(float(sigma_threshold)):
        raise ValueError("%s: sigma_threshold is NaN" % who)
    if int(dilate) != dilate or int(dilate) < 0:
        raise ValueError("%s: dilate must be an integer >= 0, got %r" % (who, dilate))
    words = (resolution ** 3 + 31) // 32
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.int32
                            or tuple(out.shape) != (words,)):
        raise ValueError("%s: out must be the (%d,) int32 words of a resolution %d grid, got %s"
                         % (who, words, resolution,
                            (out.dtype, tuple(out.shape)) if torch.is_tensor(out) else type(out).__name__))
    return words


def occupancy_from_octree(leaf_index: torch.Tensor, scale: float, center, box_min, box_size,
                          resolution: int, rows: Optional[torch.Tensor] = None, stride: int = 4,
                          sigma_offset: int = 3, sigma_threshold: Optional[float] = None,
                          dilate: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K25.  The boxes of an octree's leaves rasterised into a K9 grid -> bit mask
    (ceil(G^3/32),) int32, as ``occupancy_build`` returns.  ``leaf_index`` (L,) int64 sorted ids,
    ``scale`` and ``center`` the root cube; ``box_min`` / ``box_size`` the grid's box.  A leaf marks
    every cell that meets its half-open box in grid coordinates (``ffn_occupancy_from_octree`` in
    include/ffn_hip.h states the rule and what it guarantees).  ``rows`` (L, stride) float32 with the
    density at ``sigma_offset`` and ``sigma_threshold``: leaves with density <= threshold mark
    nothing (NaN marks); without ``rows`` every leaf marks.  ``dilate`` = n passes of the
    26-neighbourhood dilation over what this call marks.  With ``out`` (a tensor this function
    returned for the same resolution) the cells are ORed into it and it is returned: leaf subsets
    or several trees folded over several calls give the bits of one call.  One device-to-host sync
    (the row count sizes the second launch).  Bad input is a ``ValueError``
    (``occupancy_from_octree_check``)."""
    words = occupancy_from_octree_check(leaf_index, scale, center, box_min, box_size, resolution,
                                        rows, stride, sigma_offset, sigma_threshold, dilate, out)
    dev = leaf_index.device
    leaves, dilate = leaf_index.shape[0], int(dilate)
    bits = out if out is not None else torch.empty((words,), dtype=torch.int32, device=dev)
    plan = torch.empty((leaves, 4), dtype=torch.int32, device=dev)
    offsets = torch.empty((leaves,), dtype=torch.int32, device=dev)
    tiles = torch.empty(((leaves + 4095) // 4096,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int64, device=dev)
    scratch = None
    if dilate > 0:
        scratch = torch.empty((words * (2 if out is not None else 1),), dtype=torch.int32, device=dev)
    use = sigma_threshold is not None
    _call("ffn_occupancy_from_octree", _dev(leaf_index, torch.int64, "leaf_index"), c_i64(leaves),
          c_f(scale), _host3(center), _dev(rows, name="rows"), c_i(int(stride)),
          c_i(int(sigma_offset)), c_f(float(sigma_threshold) if use else 0.0), c_i(1 if use else 0),
          _host3(box_min), _host3(box_size), c_i(int(resolution)), c_i(0 if out is None else 1),
          c_i(dilate), _dev(plan, torch.int32, "plan"), _dev(offsets, torch.int32, "offsets"),
          _dev(tiles, torch.int32, "tiles"),
          _dev(total, torch.int64, "total"), _dev(scratch, torch.int32), _dev(bits, torch.int32, "out"))
    return bits


def scatter_logits(packed: torch.Tensor, index: torch.Tensor, n: int,
                   empty_sigma_logit: float = -100.0) -> torch.Tensor:
    """K9f.  (M,4) logits of the evaluated samples -> (N,4), the rest (0,0,0,empty_sigma_logit)."""
    _want("scatter_logits", "packed", packed, (None, 4))
    _want("scatter_logits", "index", index, (packed.shape[0],), torch.int32)
    _want_int("scatter_logits", "n", n, packed.shape[0])
    out = torch.empty((n, 4), dtype=torch.float32, device=index.device)
    _call("ffn_scatter_logits", _dev(packed), _dev(index, torch.int32), c_i64(packed.shape[0]),
              c_i64(n), c_f(empty_sigma_logit), _dev(out))
    return out


def gather_logits(full: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    """K9g.  (N,4) rows at ``index`` (int32) -> (M,4)."""
    _want("gather_logits", "full", full, (None, 4))
    _want("gather_logits", "index", index, (None,), torch.int32)
    m = index.shape[0]
    out = torch.empty((m, 4), dtype=torch.float32, device=full.device)
    if m > 0:
        _call("ffn_gather_logits", _dev(full), _dev(index, torch.int32), c_i64(m), _dev(out))
    return out


# --------------------------------------------------------------------------------- voxels
def voxels_forward(volume: torch.Tensor, bias: torch.Tensor, positions: torch.Tensor, side: int,
                   scale: float) -> torch.Tensor:
    """K10.  volume (4,S,S,S), bias (4), positions (N,3) -> logits (N,4)."""
    _want_int("voxels_forward", "side", side, 1)
    _want_numel("voxels_forward", "volume", volume, 4 * side ** 3)
    _want_numel("voxels_forward", "bias", bias, 4)
    _want("voxels_forward", "positions", positions, (None, 3))
    n = positions.shape[0]
    out = torch.empty((n, 4), dtype=torch.float32, device=positions.device)
    _call("ffn_voxels_forward", _dev(volume), _dev(bias), _dev(positions, name="positions"),
              c_i64(n), c_i(side), c_f(scale), _dev(out))
    return out


def voxels_backward_workspace_bytes(n: int, side: int) -> int:
    """Bytes of workspace ``voxels_backward`` needs for ``n`` samples of a side-``side`` volume."""
    fn = _lib.load().ffn_voxels_backward_workspace
    fn.restype = ctypes.c_int64
    size = fn(c_i64(n), c_i(side))
    if size < 0:
        raise _lib.FfnError("ffn_voxels_backward_workspace failed: %s"
                            % _lib.load().ffn_last_error_string().decode())
    return int(size)


def voxels_backward(positions: torch.Tensor, d_logits: torch.Tensor, side: int, scale: float,
                    workspace: Optional[torch.Tensor] = None, d_volume: Optional[torch.Tensor] = None,
                    d_bias: Optional[torch.Tensor] = None):
    """K10b, the adjoint of K10.  positions (N,3), d_logits (N,4) -> d_volume (4,S,S,S) and
    d_bias (4), both overwritten (no zeroing needed); deterministic (no float atomics).
    ``workspace``: any float32 device tensor of at least ``voxels_backward_workspace_bytes``."""
    who = "voxels_backward"
    _want_int(who, "side", side, 1, 1024)
    _want(who, "positions", positions, (None, 3))
    n = positions.shape[0]
    _want(who, "d_logits", d_logits, (n, 4))
    dev = positions.device
    need = voxels_backward_workspace_bytes(n, side)
    if workspace is not None:
        _want_numel(who, "workspace", workspace, (need + 3) // 4, at_least=True)
    if workspace is None:
        workspace = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=dev)
    if d_volume is None:
        d_volume = torch.empty((4, side, side, side), dtype=torch.float32, device=dev)
    if d_bias is None:
        d_bias = torch.empty((4,), dtype=torch.float32, device=dev)
    if d_volume.numel() != 4 * side ** 3 or d_bias.numel() != 4:
        raise ValueError("voxels_backward: d_volume must hold 4*side^3 floats and d_bias 4")
    _call("ffn_voxels_backward", _dev(positions, name="positions"), _dev(d_logits, name="d_logits"),
          c_i64(n), c_i(side), c_f(scale), _dev(workspace), c_i64(workspace.numel() * 4),
          _dev(d_volume), _dev(d_bias))
    return d_volume, d_bias


# --------------------------------------------------------------------------------- octree
def octree_max_depth() -> int:
    """The deepest ``voxel_depth`` the K12 path codes hold."""
    fn = _lib.load().ffn_octree_max_depth
    fn.restype = ctypes.c_int
    return int(fn())


def _scan_scratch(elements: int, device):
    """flags, offsets, tile_sums for a K12 flag scan over ``elements`` flags."""
    fn = _lib.load().ffn_octree_scan_tiles
    fn.restype = ctypes.c_int64
    tiles = int(fn(c_i64(elements)))
    return (torch.empty((elements,), dtype=torch.uint8, device=device),
            torch.empty((elements,), dtype=torch.int32, device=device),
            torch.empty((max(tiles, 1),), dtype=torch.int32, device=device))


def octree_surface_points(alpha: torch.Tensor, depth: torch.Tensor, starts: torch.Tensor,
                          directions: torch.Tensor, threshold: float,
                          color: Optional[torch.Tensor] = None):
    """K12a-d.  alpha (N), depth (N), starts (N,3), directions (N,3), color (N,C) or None ->
    positions (N,3), colors (N,C) or None, count (int32 scalar on the device): the first
    ``count`` rows hold ``starts + directions * depth`` / ``color`` of the rays with
    ``alpha > threshold``, in ray order; the other rows are zero."""
    who = "octree_surface_points"
    _want(who, "alpha", alpha, (None,))
    n = alpha.shape[0]
    if color is not None:
        _want(who, "color", color, (n, None))
    if n > 0:
        _want(who, "depth", depth, (n,))
        _want(who, "starts", starts, (n, 3))
        _want(who, "directions", directions, (n, 3))
    dev = alpha.device
    channels = 0 if color is None else color.shape[1]
    # zeros, not empty: the rows past ``count`` are returned too, and whatever an earlier tensor
    # left in recycled memory (a NaN, say) must not show up in them
    out_pos = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    out_col = None if color is None else torch.zeros((n, channels), dtype=torch.float32, device=dev)
    count = torch.zeros((), dtype=torch.int32, device=dev)
    if n == 0:
        return out_pos, out_col, count
    if depth.shape[0] != n or starts.shape != (n, 3) or directions.shape != (n, 3):
        raise ValueError("octree_surface_points: alpha, depth, starts, directions disagree on N")
    flags, offsets, tiles = _scan_scratch(n, dev)
    _call("ffn_octree_surface_points", _dev(alpha, name="alpha"), _dev(depth, name="depth"),
          _dev(starts, name="starts"), _dev(directions, name="directions"),
          _dev(color, name="color"), c_i64(n), c_i(channels), c_f(threshold),
          _dev(flags, torch.uint8), _dev(offsets, torch.int32), _dev(tiles, torch.int32),
          _dev(out_pos), _dev(out_col), _dev(count, torch.int32))
    return out_pos, out_col, count


def octree_path_codes(positions: torch.Tensor, center, scale: float, depth: int) -> torch.Tensor:
    """K12e.  positions (N,3), the cube's centre (3 floats) and half side -> int32 codes (N)."""
    _want("octree_path_codes", "positions", positions, (None, 3))
    n = positions.shape[0]
    codes = torch.empty((n,), dtype=torch.int32, device=positions.device)
    if n == 0:
        return codes
    _call("ffn_octree_path_codes", _dev(positions, name="positions"), c_i64(n), c_f(center[0]),
          c_f(center[1]), c_f(center[2]), c_f(scale), c_i(depth), _dev(codes, torch.int32))
    return codes


def octree_structure(sorted_codes: torch.Tensor, perm: torch.Tensor, depth: int,
                     min_leaf_size: int):
    """K12f-g on stably sorted codes.  -> leaf_of_point (N) int64 (leaf id or -1, in the caller's
    point order), and per leaf in code order: leaf_ids (L) int64, leaf_start (L) int64,
    leaf_count (L) int32.  Reads the leaf count back once."""
    who = "octree_structure"
    _want(who, "sorted_codes", sorted_codes, (None,), torch.int32)
    _want(who, "perm", perm, (sorted_codes.shape[0],), torch.int64)
    n = sorted_codes.shape[0]
    dev = sorted_codes.device
    leaf_sorted = torch.empty((n,), dtype=torch.int64, device=dev)
    count_sorted = torch.empty((n,), dtype=torch.int32, device=dev)
    leaf_of_point = torch.empty((n,), dtype=torch.int64, device=dev)
    leaf_ids = torch.empty((n,), dtype=torch.int64, device=dev)
    leaf_start = torch.empty((n,), dtype=torch.int64, device=dev)
    leaf_count = torch.empty((n,), dtype=torch.int32, device=dev)
    num = torch.zeros((), dtype=torch.int32, device=dev)
    if n == 0:
        return leaf_of_point, leaf_ids, leaf_start, leaf_count
    flags, offsets, tiles = _scan_scratch(n, dev)
    _call("ffn_octree_structure", _dev(sorted_codes, torch.int32, "sorted_codes"),
          _dev(perm, torch.int64, "perm"), c_i64(n), c_i(depth), c_i64(min_leaf_size),
          _dev(leaf_sorted, torch.int64), _dev(count_sorted, torch.int32),
          _dev(leaf_of_point, torch.int64), _dev(flags, torch.uint8), _dev(offsets, torch.int32),
          _dev(tiles, torch.int32), _dev(leaf_ids, torch.int64), _dev(leaf_start, torch.int64),
          _dev(leaf_count, torch.int32), _dev(num, torch.int32))
    k = int(num.item())
    return leaf_of_point, leaf_ids[:k].clone(), leaf_start[:k].clone(), leaf_count[:k].clone()


def octree_interior_nodes(leaf_ids: torch.Tensor, depth: int) -> torch.Tensor:
    """K12h.  leaf ids in code order -> the ids of the interior nodes (int64, unsorted)."""
    _want("octree_interior_nodes", "leaf_ids", leaf_ids, (None,), torch.int64)
    k = leaf_ids.shape[0]
    dev = leaf_ids.device
    if depth < 2 or k == 0:
        return torch.empty((0,), dtype=torch.int64, device=dev)
    m = k * (depth - 1)
    flags, offsets, tiles = _scan_scratch(m, dev)
    nodes = torch.empty((m,), dtype=torch.int64, device=dev)
    num = torch.zeros((), dtype=torch.int32, device=dev)
    _call("ffn_octree_interior_nodes", _dev(leaf_ids, torch.int64, "leaf_ids"), c_i64(k),
          c_i(depth), _dev(flags, torch.uint8), _dev(offsets, torch.int32),
          _dev(tiles, torch.int32), _dev(nodes, torch.int64), _dev(num, torch.int32))
    return nodes[:int(num.item())].clone()


def octree_leaf_means(data: torch.Tensor, perm: torch.Tensor, leaf_start: torch.Tensor,
                      leaf_count: torch.Tensor) -> torch.Tensor:
    """K12i.  data (N,C), perm (N) int64, per leaf start / count into perm -> (L,C) means."""
    who = "octree_leaf_means"
    _want(who, "data", data, (None, None))
    _want(who, "perm", perm, (data.shape[0],), torch.int64)
    _want(who, "leaf_start", leaf_start, (None,), torch.int64)
    _want(who, "leaf_count", leaf_count, (leaf_start.shape[0],), torch.int32)
    k = leaf_start.shape[0]
    n, channels = data.shape
    out = torch.empty((k, channels), dtype=torch.float32, device=data.device)
    if k > 0:
        _call("ffn_octree_leaf_means", _dev(data, name="data"), c_i64(n), c_i(channels),
              _dev(perm, torch.int64, "perm"), _dev(leaf_start, torch.int64, "leaf_start"),
              _dev(leaf_count, torch.int32, "leaf_count"), c_i64(k), _dev(out))
    return out


def octree_query(positions: torch.Tensor, scale: float, node_index: torch.Tensor,
                 leaf_index: torch.Tensor) -> torch.Tensor:
    """K12j.  positions (N,3), sorted int64 id arrays -> (N) int64 index into leaf_index or -1."""
    _want("octree_query", "positions", positions, (None, 3))
    _want("octree_query", "node_index", node_index, (None,), torch.int64)
    _want("octree_query", "leaf_index", leaf_index, (None,), torch.int64)
    n = positions.shape[0]
    out = torch.empty((n,), dtype=torch.int64, device=positions.device)
    if n > 0:
        _call("ffn_octree_query", _dev(positions, name="positions"), c_i64(n), c_f(scale),
              _dev(node_index if node_index.numel() else None, torch.int64, "node_index"),
              c_i64(node_index.numel()), _dev(leaf_index, torch.int64, "leaf_index"),
              c_i64(leaf_index.numel()), _dev(out, torch.int64))
    return out


def octree_leaf_geometry(leaf_index: torch.Tensor, scale: float):
    """K12k.  sorted leaf ids -> centres (L,3) float32 and depths (L) int32."""
    _want("octree_leaf_geometry", "leaf_index", leaf_index, (None,), torch.int64)
    k = leaf_index.shape[0]
    centers = torch.empty((k, 3), dtype=torch.float32, device=leaf_index.device)
    depths = torch.empty((k,), dtype=torch.int32, device=leaf_index.device)
    if k > 0:
        _call("ffn_octree_leaf_geometry", _dev(leaf_index, torch.int64, "leaf_index"), c_i64(k),
              c_f(scale), _dev(centers), _dev(depths, torch.int32))
    return centers, depths


def _walk_check(starts, directions, scale, depth, node_index, leaf_index):
    """What every walk refuses: rays that are not (N,3) twice, id arrays that are not (n,) int64, a
    depth outside 1 .. 11 (include/ffn_hip.h, K13)."""
    if not isinstance(starts, torch.Tensor) or not isinstance(directions, torch.Tensor) \
            or starts.dim() != 2:
        raise ValueError("octree walk: starts and directions must both be (N,3)")
    n = starts.shape[0]
    if starts.shape != (n, 3) or directions.shape != (n, 3):
        raise ValueError("octree walk: starts and directions must both be (N,3)")
    _want("octree walk", "node_index", node_index, (None,), torch.int64)
    _want("octree walk", "leaf_index", leaf_index, (None,), torch.int64)
    _want_int("octree walk", "depth", depth, 1, 11)


def _walk_args(starts, directions, scale, depth, node_index, leaf_index):
    _walk_check(starts, directions, scale, depth, node_index, leaf_index)
    n = starts.shape[0]
    return (_dev(starts, name="starts"), _dev(directions, name="directions"), c_i64(n),
            c_f(scale), c_i(depth),
            _dev(node_index if node_index.numel() else None, torch.int64, "node_index"),
            c_i64(node_index.numel()), _dev(leaf_index, torch.int64, "leaf_index"),
            c_i64(leaf_index.numel()))


def octree_walk(starts: torch.Tensor, directions: torch.Tensor, scale: float, depth: int,
                node_index: torch.Tensor, leaf_index: torch.Tensor, max_length: int):
    """K13.  starts, directions (N,3) in the tree's frame, sorted int64 id arrays, depth = 1 + the
    deepest leaf's level -> t_stops (N,max_length) float32, leaves (N,max_length) int64."""
    _walk_check(starts, directions, scale, depth, node_index, leaf_index)
    _want_int("octree walk", "max_length", max_length, 2)
    n = starts.shape[0]
    t_stops = torch.empty((n, max_length), dtype=torch.float32, device=starts.device)
    leaves = torch.empty((n, max_length), dtype=torch.int64, device=starts.device)
    if n > 0:
        _call("ffn_octree_walk", *_walk_args(starts, directions, scale, depth, node_index,
                                             leaf_index),
              c_i(max_length), _dev(t_stops), _dev(leaves, torch.int64))
    return t_stops, leaves


def octree_spans(starts: torch.Tensor, directions: torch.Tensor, scale: float, depth: int,
                 node_index: torch.Tensor, leaf_index: torch.Tensor, t_min: float = 0.0,
                 pad: float = 1.0):
    """K13, span form.  -> t_in (N), t_out (N) float32 and hit (N) uint8: the span of the leaves
    that end after ``t_min``, widened by ``pad`` finest-cell sides along the ray."""
    _walk_check(starts, directions, scale, depth, node_index, leaf_index)
    n = starts.shape[0]
    t_in = torch.empty((n,), dtype=torch.float32, device=starts.device)
    t_out = torch.empty((n,), dtype=torch.float32, device=starts.device)
    hit = torch.empty((n,), dtype=torch.uint8, device=starts.device)
    if n > 0:
        _call("ffn_octree_spans", *_walk_args(starts, directions, scale, depth, node_index,
                                              leaf_index),
              c_f(t_min), c_f(pad), _dev(t_in), _dev(t_out), _dev(hit, torch.uint8))
    return t_in, t_out, hit


OCTREE_SHADING = {"flat": 0, "faces": 1}      # FFN_OCTREE_SHADING_* of include/ffn_hip.h


def octree_face_shade():
    """The seven factors of ``"faces"`` shading (FFN_OCTREE_FACE_SHADE), as the library holds
    them: one per entry face 0 .. 5 and 1.0 for face 6 -> numpy float32 (7,)."""
    table = (ctypes.c_float * 7)()
    fn = _lib.load().ffn_octree_face_shade
    fn.restype = None
    fn(table)
    return np.array(list(table), dtype=np.float32)


def octree_first_hit(starts: torch.Tensor, directions: torch.Tensor, scale: float, depth: int,
                     node_index: torch.Tensor, leaf_index: torch.Tensor, t_min: float = 0.0):
    """K14.  Arguments as for ``octree_spans`` -> per ray the first leaf that ends after ``t_min``:
    leaf (N) int64 index into leaf_index or -1, t_hit (N) float32 = max(entry t, t_min) or 0,
    face (N) int8: the entry face 0 .. 5, 6 for an entry before ``t_min``, -1 for a miss."""
    _walk_check(starts, directions, scale, depth, node_index, leaf_index)
    n = starts.shape[0]
    leaf = torch.empty((n,), dtype=torch.int64, device=starts.device)
    t_hit = torch.empty((n,), dtype=torch.float32, device=starts.device)
    face = torch.empty((n,), dtype=torch.int8, device=starts.device)
    if n > 0:
        _call("ffn_octree_first_hit", *_walk_args(starts, directions, scale, depth, node_index,
                                                  leaf_index),
              c_f(t_min), _dev(leaf, torch.int64), _dev(t_hit), _dev(face, torch.int8))
    return leaf, t_hit, face


def octree_render(starts: torch.Tensor, directions: torch.Tensor, scale: float, depth: int,
                  node_index: torch.Tensor, leaf_index: torch.Tensor, leaf_data: torch.Tensor,
                  t_min: float = 0.0, background=(0.0, 0.0, 0.0), shading: str = "flat",
                  want_hit: bool = False):
    """K14, shaded in the same launch.  leaf_data (L,C) float32 with C >= 3 -> color (N,3),
    alpha (N) (1 on a hit, 0 otherwise), depth (N) = t_hit; misses carry ``background``.
    ``shading``: "flat" or "faces".  With ``want_hit`` also the (leaf, t_hit, face) of
    ``octree_first_hit``."""
    if shading not in OCTREE_SHADING:
        raise ValueError("octree render: shading is 'flat' or 'faces', got %r" % (shading,))
    _walk_check(starts, directions, scale, depth, node_index, leaf_index)
    if not isinstance(leaf_data, torch.Tensor):
        raise ValueError("octree render: leaf_data must be a tensor, got %s"
                         % type(leaf_data).__name__)
    if leaf_data.dim() != 2 or leaf_data.shape[0] != leaf_index.numel() or leaf_data.shape[1] < 3:
        raise ValueError("octree render: leaf_data must be (num_leaves, C >= 3), got %s for %d "
                         "leaves" % (tuple(leaf_data.shape), leaf_index.numel()))
    n = starts.shape[0]
    dev = starts.device
    color = torch.empty((n, 3), dtype=torch.float32, device=dev)
    alpha = torch.empty((n,), dtype=torch.float32, device=dev)
    depth_out = torch.empty((n,), dtype=torch.float32, device=dev)
    hit = None
    if want_hit:
        hit = (torch.empty((n,), dtype=torch.int64, device=dev),
               torch.empty((n,), dtype=torch.float32, device=dev),
               torch.empty((n,), dtype=torch.int8, device=dev))
    if n > 0:
        r, g, b = [float(v) for v in background]
        _call("ffn_octree_render", *_walk_args(starts, directions, scale, depth, node_index,
                                               leaf_index),
              c_f(t_min), _dev(leaf_data, name="leaf_data"), c_i(leaf_data.shape[1]), c_f(r),
              c_f(g), c_f(b), c_i(OCTREE_SHADING[shading]), _dev(color), _dev(alpha),
              _dev(depth_out), _dev(hit[0] if hit else None, torch.int64),
              _dev(hit[1] if hit else None), _dev(hit[2] if hit else None, torch.int8))
    if want_hit:
        return color, alpha, depth_out, hit
    return color, alpha, depth_out


def _check_leaf_data(who, leaf_data, leaf_index):
    for name, t in (("leaf_index", leaf_index), ("leaf_data", leaf_data)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
    if leaf_data.dim() != 2 or leaf_data.shape[0] != leaf_index.numel() or leaf_data.shape[1] < 4:
        raise ValueError("%s: leaf_data must be (num_leaves, C >= 4), got %s for %d leaves"
                         % (who, tuple(leaf_data.shape), leaf_index.numel()))


def _check_min_transmittance(who, min_transmittance):
    if not 0.0 <= min_transmittance < 1.0:
        raise ValueError("%s: min_transmittance must lie in [0, 1), got %r"
                         % (who, min_transmittance,))


def _render_volume(name, walk, t_min, leaf_block, background, min_transmittance, tail=()):
    """A volume render through entry point ``name`` -> color (N,3), alpha (N), depth (N).
    ``walk``: the arguments of ``_walk_args``; ``leaf_block()``: the leaf arguments after
    ``t_min``; ``tail``: those after the outputs."""
    _walk_check(*walk)
    n, dev = walk[0].shape[0], walk[0].device
    color = torch.empty((n, 3), dtype=torch.float32, device=dev)
    alpha = torch.empty((n,), dtype=torch.float32, device=dev)
    depth_out = torch.empty((n,), dtype=torch.float32, device=dev)
    if n > 0:
        r, g, b = [float(v) for v in background]
        _call(name, *_walk_args(*walk), c_f(t_min), *leaf_block(), c_f(r), c_f(g), c_f(b),
              c_f(min_transmittance), _dev(color), _dev(alpha), _dev(depth_out), *tail)
    return color, alpha, depth_out


def octree_render_volume(starts: torch.Tensor, directions: torch.Tensor, scale: float, depth: int,
                         node_index: torch.Tensor, leaf_index: torch.Tensor,
                         leaf_data: torch.Tensor, t_min: float = 0.0,
                         background=(0.0, 0.0, 0.0), min_transmittance: float = 0.0):
    """K15.  leaf_data (L,C) float32 with C >= 4, [r, g, b, sigma, ...] as ``octree_bake`` makes
    them -> color (N,3), alpha (N), depth (N), composited front to back over the leaves every ray
    crosses after ``t_min``; the walk of a ray ends once its transmittance is at or below
    ``min_transmittance``."""
    _check_leaf_data("octree render_volume", leaf_data, leaf_index)
    _check_min_transmittance("octree render_volume", min_transmittance)
    return _render_volume("ffn_octree_render_volume",
                          (starts, directions, scale, depth, node_index, leaf_index), t_min,
                          lambda: (_dev(leaf_data, name="leaf_data"), c_i(leaf_data.shape[1])),
                          background, min_transmittance)


def octree_sh_channels(degree: int) -> int:
    """3 (degree + 1)^2 + 1: the channels of an SH leaf; degree is 1 or 2."""
    if degree not in (1, 2) or isinstance(degree, bool):
        raise ValueError("octree SH: degree is 1 or 2, got %r" % (degree,))
    return 3 * (degree + 1) ** 2 + 1


def octree_sh_device_layout(leaf_data: np.ndarray, degree: int) -> np.ndarray:
    """(L, 3B+1) in the file's order [k_r.., k_g.., k_b.., sigma] -> the float32 rows K18a reads:
    [sigma, k_r.., k_g.., k_b.., 0 ..], the row stride padded to a multiple of four floats."""
    channels = octree_sh_channels(degree)
    if np.ndim(leaf_data) != 2 or np.shape(leaf_data)[1] != channels:
        raise ValueError("octree SH: leaf_data must be (num_leaves, %d) for degree %d, got %s"
                         % (channels, degree, np.shape(leaf_data),))
    stride = (channels + 3) // 4 * 4
    rows = np.zeros((len(leaf_data), stride), np.float32)
    rows[:, 0] = leaf_data[:, channels - 1]
    rows[:, 1:channels] = leaf_data[:, :channels - 1]
    return rows


def _check_leaf_rows(who, leaf_rows, leaf_index, degree) -> int:
    """SH rows in the device layout, one per leaf -> the channels of ``degree``."""
    channels = octree_sh_channels(degree)
    for name, t in (("leaf_index", leaf_index), ("leaf_rows", leaf_rows)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a tensor, got %s" % (who, name, type(t).__name__))
    if (leaf_rows.dim() != 2 or leaf_rows.shape[0] != leaf_index.numel()
            or leaf_rows.shape[1] < channels or leaf_rows.shape[1] % 4 != 0):
        raise ValueError("%s: leaf_rows must be (num_leaves, stride) with stride a multiple of 4 "
                         "and >= %d, got %s for %d leaves"
                         % (who, channels, tuple(leaf_rows.shape), leaf_index.numel()))
    return channels


def octree_render_volume_sh(starts: torch.Tensor, directions: torch.Tensor, scale: float,
                            depth: int, node_index: torch.Tensor, leaf_index: torch.Tensor,
                            leaf_rows: torch.Tensor, degree: int, t_min: float = 0.0,
                            background=(0.0, 0.0, 0.0), min_transmittance: float = 0.0):
    """K18a.  ``octree_render_volume`` with a view-dependent leaf colour: leaf_rows (L, stride)
    float32 in the device layout of ``octree_sh_device_layout`` -> color (N,3), alpha (N),
    depth (N)."""
    channels = _check_leaf_rows("octree render_volume_sh", leaf_rows, leaf_index, degree)
    _check_min_transmittance("octree render_volume_sh", min_transmittance)
    return _render_volume("ffn_octree_render_volume_sh",
                          (starts, directions, scale, depth, node_index, leaf_index), t_min,
                          lambda: (_dev(leaf_rows, name="leaf_rows"), c_i(channels)), background,
                          min_transmittance, (c_i(degree), c_i(leaf_rows.shape[1])))


def octree_sh_accumulate(logits: torch.Tensor, leaf_data: torch.Tensor, weights, inv_views: float,
                         degree: int) -> torch.Tensor:
    """K18b, in place on leaf_data (L, 3B+1) (file layout): one view's logits (L,4) times that
    view's B projection weights (host floats) into the coefficients, softplus(sigma logit) *
    inv_views into the density."""
    channels = octree_sh_channels(degree)
    basis = (channels - 1) // 3
    for name, t in (("logits", logits), ("leaf_data", leaf_data)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("octree sh_accumulate: %s must be a tensor, got %s"
                             % (name, type(t).__name__))
    if logits.dim() != 2 or logits.shape[1] != 4:
        raise ValueError("octree sh_accumulate: logits must be (L,4), got %s"
                         % (tuple(logits.shape),))
    if leaf_data.dim() != 2 or tuple(leaf_data.shape) != (logits.shape[0], channels):
        raise ValueError("octree sh_accumulate: leaf_data must be (%d, %d), got %s"
                         % (logits.shape[0], channels, tuple(leaf_data.shape)))
    weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    if len(weights) != basis:
        raise ValueError("octree sh_accumulate: %d weights for degree %d, got %d"
                         % (basis, degree, len(weights)))
    if logits.shape[0] > 0:
        host = (ctypes.c_float * basis)(*[float(v) for v in weights])
        _call("ffn_octree_sh_accumulate", _dev(logits, name="logits"), c_i64(logits.shape[0]),
              c_i(degree), host, c_f(inv_views), _dev(leaf_data, name="leaf_data"))
    return leaf_data


def _grad_workspace_bytes(name, *args):
    fn = getattr(_lib.load(), name)
    fn.restype = ctypes.c_int64
    size = fn(*args)
    if size < 0:
        raise _lib.FfnError("%s failed: %s" % (name, _lib.load().ffn_last_error_string().decode()))
    return int(size)


def octree_grad_dist_workspace_bytes(n: int, num_leaves: int, max_entries: int,
                                     degree: int = 0) -> int:
    """Bytes of workspace the backwards need with the distortion term (K29b) switched on: those of
    ``octree_grad_workspace_bytes`` (``degree`` 0) or ``octree_grad_sh_workspace_bytes`` plus three
    floats per ray."""
    return _grad_workspace_bytes("ffn_octree_grad_dist_workspace_bytes", c_i64(n),
                                 c_i64(num_leaves), c_i64(max_entries), c_i(degree))


def octree_grad_workspace_bytes(n: int, num_leaves: int, max_entries: int) -> int:
    """Bytes of workspace ``octree_render_volume_backward`` needs for ``n`` rays, ``num_leaves``
    leaves and up to ``max_entries`` (ray, taken leaf) pairs."""
    return _grad_workspace_bytes("ffn_octree_grad_workspace_bytes", c_i64(n), c_i64(num_leaves),
                                 c_i64(max_entries))


class OctreeGradWorkspace:
    """The workspace of K17b, kept between calls and grown when the rays take more leaves than
    it holds (``entries_per_ray`` is the first guess)."""

    def __init__(self, entries_per_ray: int = 32):
        self.entries_per_ray = int(entries_per_ray)
        self.max_entries = 0
        self.buffer = None
        self.shape = None
        self.entries = 0            # of the last call
        self.dist = False           # K29b: the buffer also holds the per-ray triples

    def _bytes(self, n, num_leaves, want):
        return octree_grad_workspace_bytes(n, num_leaves, want)

    def _dist_bytes(self, n, num_leaves, want):
        return octree_grad_dist_workspace_bytes(n, num_leaves, want, getattr(self, "degree", 0))

    def fit(self, n: int, num_leaves: int, device, at_least: int = 0, dist: bool = False):
        same = (self.buffer is not None and self.shape == (n, num_leaves)
                and self.buffer.device == device and (self.dist or not dist))
        if same and self.max_entries >= max(at_least, 1):
            return
        if at_least > 0:
            self.entries_per_ray = max(self.entries_per_ray, -(-at_least // n))
        want = max(at_least, n * self.entries_per_ray, 1024)
        need = (self._dist_bytes if dist else self._bytes)(n, num_leaves, want)
        self.dist = bool(dist)
        if self.buffer is None or self.buffer.numel() * 4 < need or self.buffer.device != device:
            self.buffer = None              # release before the larger one is taken
            self.buffer = torch.empty(((need + 3) // 4,), dtype=torch.float32, device=device)
        self.max_entries = want
        self.shape = (n, num_leaves)


def octree_check_dist_scale(who, dist_scale) -> float:
    """A weight of the distortion term (K29): a finite float >= 0, else ``ValueError`` naming it."""
    try:
        value = float(dist_scale)
    except (TypeError, ValueError):
        value = float("nan")
    if isinstance(dist_scale, bool) or not (math.isfinite(value) and value >= 0.0):
        raise ValueError("%s must be finite and >= 0, got %r" % (who, dist_scale))
    return value


def _render_volume_backward(name, walk, t_min, leaf_block, background, min_transmittance, grads,
                            workspace, out, width, degree=None, tail=(), dist=None):
    """The backward of a volume render through entry point ``name``: the output (num_leaves,
    ``width``), the call on ``workspace`` and, when the rays take more leaves than it holds, its
    growth and ONE repeat.  ``walk``: the arguments of ``_walk_args``; ``leaf_block()``: the leaf
    arguments after ``t_min``; ``tail``: those after ``entries``; ``degree``: of SH rows.
    ``dist = (dist_scale, ray_distortion)`` (K29b) calls entry point ``name + "_dist"`` with the two
    behind ``tail``; ``None`` calls ``name`` as ever."""
    who = "octree " + name[len("ffn_octree_"):]
    _walk_check(*walk)
    starts, leaf_index = walk[0], walk[5]
    d_color, d_alpha = grads
    for label, t in (("d_color", d_color), ("d_alpha", d_alpha)):
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a tensor, got %s" % (who, label, type(t).__name__))
    n, leaves = starts.shape[0], leaf_index.numel()
    if d_color.shape != (n, 3) or d_alpha.shape != (n,):
        raise ValueError("%s: d_color must be (N,3) and d_alpha (N,)" % who)
    dev = starts.device
    if out is None:
        out = torch.empty((leaves, width), dtype=torch.float32, device=dev)
    if out.shape != (leaves, width):
        raise ValueError("%s: %s must be (num_leaves, %d)"
                         % (who, "d_leaf_data" if degree is None else "d_leaf_rows", width))
    if dist is not None:
        dist_scale, ray_distortion = dist
        if ray_distortion is not None and ray_distortion.shape != (n,):
            raise ValueError("%s: ray_distortion must be (N,) = (%d,), got %s"
                             % (who, n, tuple(ray_distortion.shape)))
        if n > 0:
            name = name + "_dist"
            tail = tuple(tail) + (c_f(dist_scale), _dev(ray_distortion, name="ray_distortion"))
    if n == 0:
        return out.zero_()
    if degree is not None and getattr(workspace, "degree", None) != degree:
        raise ValueError("%s: the workspace is not one of degree %d" % (who, degree))
    r, g, b = [float(v) for v in background]
    entries = c_i64(-1)
    workspace.fit(n, leaves, dev, dist=dist is not None)
    for attempt in range(2):
        try:
            _call(name, *_walk_args(*walk), c_f(t_min), *leaf_block(), c_f(r), c_f(g), c_f(b),
                  c_f(min_transmittance), _dev(d_color, name="d_color"),
                  _dev(d_alpha, name="d_alpha"), _dev(workspace.buffer),
                  c_i64(workspace.buffer.numel() * 4), c_i64(workspace.max_entries), _dev(out),
                  ctypes.byref(entries), *tail)
            break
        except _lib.FfnError:
            if attempt == 1 or entries.value <= workspace.max_entries:
                raise
            workspace.fit(n, leaves, dev, at_least=entries.value + entries.value // 4,
                          dist=dist is not None)
    workspace.entries = int(entries.value)
    return out


def octree_render_volume_backward(starts: torch.Tensor, directions: torch.Tensor, scale: float,
                                  depth: int, node_index: torch.Tensor, leaf_index: torch.Tensor,
                                  leaf_data: torch.Tensor, d_color: torch.Tensor,
                                  d_alpha: torch.Tensor, t_min: float = 0.0,
                                  background=(0.0, 0.0, 0.0), min_transmittance: float = 0.0,
                                  workspace: Optional[OctreeGradWorkspace] = None,
                                  d_leaf_data: Optional[torch.Tensor] = None,
                                  dist_scale: float = 0.0,
                                  ray_distortion: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K17a + K17b, the backward of ``octree_render_volume``: d_color (N,3), d_alpha (N) ->
    d_leaf_data (L,4) float32 [d r, d g, d b, d sigma], every row written, deterministic (no float
    atomics).  One read-back (the number of (ray, taken leaf) pairs) per call; when the workspace
    turns out too small for them it is grown and the call repeated.

    K29b: with ``dist_scale > 0`` the d sigma column also holds ``dist_scale`` times the gradient of
    the rays' summed distortion (``octree_distortion``), folded into the same two walks, and
    ``ray_distortion`` (N,) float32, where given, receives ``D`` per ray with the bits of
    ``octree_distortion``.  With ``dist_scale == 0`` and no ``ray_distortion`` the entry point
    without the term is called: the bits are those of before the term existed."""
    who = "octree render_volume_backward"
    _check_leaf_data(who, leaf_data, leaf_index)
    _check_min_transmittance(who, min_transmittance)
    dist_scale = octree_check_dist_scale(who + ": dist_scale", dist_scale)
    dist = None if dist_scale == 0.0 and ray_distortion is None else (dist_scale, ray_distortion)
    if workspace is None:
        workspace = OctreeGradWorkspace()
    return _render_volume_backward(
        "ffn_octree_render_volume_backward",
        (starts, directions, scale, depth, node_index, leaf_index), t_min,
        lambda: (_dev(leaf_data, name="leaf_data"), c_i(leaf_data.shape[1])), background,
        min_transmittance, (d_color, d_alpha), workspace, d_leaf_data, 4, dist=dist)


def octree_project(leaf_data: torch.Tensor) -> torch.Tensor:
    """K17c, in place on leaf_data (L,4): rgb clamped to [0, 1], sigma to [0, inf), NaN -> 0."""
    _want_tensors("octree project", leaf_data=leaf_data)
    if leaf_data.dim() != 2 or leaf_data.shape[1] != 4:
        raise ValueError("octree project: leaf_data must be (L,4), got %s" % (tuple(leaf_data.shape),))
    if leaf_data.shape[0] > 0:
        _call("ffn_octree_project", _dev(leaf_data, name="leaf_data"), c_i64(leaf_data.shape[0]))
    return leaf_data


def octree_sh_file_layout(leaf_rows: np.ndarray, degree: int) -> np.ndarray:
    """The inverse of ``octree_sh_device_layout``: (L, stride >= 3B+1) device rows
    [sigma, k_r.., k_g.., k_b.., padding] -> (L, 3B+1) float32 in the file's order
    [k_r.., k_g.., k_b.., sigma]; the padding is dropped."""
    channels = octree_sh_channels(degree)
    if np.ndim(leaf_rows) != 2 or np.shape(leaf_rows)[1] < channels or np.shape(leaf_rows)[1] % 4:
        raise ValueError("octree SH: leaf_rows must be (num_leaves, stride) with stride a multiple "
                         "of 4 and >= %d for degree %d, got %s"
                         % (channels, degree, np.shape(leaf_rows),))
    data = np.empty((len(leaf_rows), channels), np.float32)
    data[:, :channels - 1] = leaf_rows[:, 1:channels]
    data[:, channels - 1] = leaf_rows[:, 0]
    return data


def octree_grad_sh_workspace_bytes(n: int, num_leaves: int, max_entries: int, degree: int) -> int:
    """Bytes of workspace ``octree_render_volume_sh_backward`` needs for ``n`` rays, ``num_leaves``
    leaves and up to ``max_entries`` (ray, taken leaf) pairs at ``degree``."""
    return _grad_workspace_bytes("ffn_octree_grad_sh_workspace_bytes", c_i64(n), c_i64(num_leaves),
                                 c_i64(max_entries), c_i(degree))


class OctreeGradSHWorkspace(OctreeGradWorkspace):
    """The workspace of K19b: ``OctreeGradWorkspace`` sized for the wide rows of ``degree``."""

    def __init__(self, degree: int, entries_per_ray: int = 32):
        super().__init__(entries_per_ray)
        octree_sh_channels(degree)
        self.degree = int(degree)

    def _bytes(self, n, num_leaves, want):
        return octree_grad_sh_workspace_bytes(n, num_leaves, want, self.degree)


def octree_render_volume_sh_backward(starts: torch.Tensor, directions: torch.Tensor, scale: float,
                                     depth: int, node_index: torch.Tensor,
                                     leaf_index: torch.Tensor, leaf_rows: torch.Tensor, degree: int,
                                     d_color: torch.Tensor, d_alpha: torch.Tensor,
                                     t_min: float = 0.0, background=(0.0, 0.0, 0.0),
                                     min_transmittance: float = 0.0,
                                     workspace: Optional[OctreeGradSHWorkspace] = None,
                                     d_leaf_rows: Optional[torch.Tensor] = None,
                                     dist_scale: float = 0.0,
                                     ray_distortion: Optional[torch.Tensor] = None
                                     ) -> torch.Tensor:
    """K19a + K19b, the backward of ``octree_render_volume_sh``: d_color (N,3), d_alpha (N) ->
    d_leaf_rows (L, stride) float32 in the device layout of ``leaf_rows`` [d sigma, d k_r..,
    d k_g.., d k_b.., 0 ..], every row written, deterministic (no float atomics).  The read-back and
    the grow-and-repeat of the workspace are those of ``octree_render_volume_backward``, and so are
    ``dist_scale`` and ``ray_distortion`` (K29b), which act on the d sigma column alone."""
    who = "octree render_volume_sh_backward"
    _check_leaf_rows(who, leaf_rows, leaf_index, degree)
    _check_min_transmittance(who, min_transmittance)
    dist_scale = octree_check_dist_scale(who + ": dist_scale", dist_scale)
    dist = None if dist_scale == 0.0 and ray_distortion is None else (dist_scale, ray_distortion)
    if workspace is None:
        workspace = OctreeGradSHWorkspace(degree)
    return _render_volume_backward(
        "ffn_octree_render_volume_sh_backward",
        (starts, directions, scale, depth, node_index, leaf_index), t_min,
        lambda: (_dev(leaf_rows, name="leaf_rows"),), background, min_transmittance,
        (d_color, d_alpha), workspace, d_leaf_rows, leaf_rows.shape[1], degree,
        (c_i(degree), c_i(leaf_rows.shape[1])), dist=dist)


def octree_project_sh(leaf_rows: torch.Tensor, degree: int) -> torch.Tensor:
    """K19c, in place on leaf_rows (L, stride) in the device layout: density to [0, inf), NaN -> 0
    for density and coefficients; the coefficients are otherwise untouched, the padding too."""
    channels = octree_sh_channels(degree)
    _want_tensors("octree project_sh", leaf_rows=leaf_rows)
    if leaf_rows.dim() != 2 or leaf_rows.shape[1] < channels or leaf_rows.shape[1] % 4 != 0:
        raise ValueError("octree project_sh: leaf_rows must be (L, stride) with stride a multiple "
                         "of 4 and >= %d, got %s" % (channels, tuple(leaf_rows.shape),))
    if leaf_rows.shape[0] > 0:
        _call("ffn_octree_project_sh", _dev(leaf_rows, name="leaf_rows"),
              c_i64(leaf_rows.shape[0]), c_i(leaf_rows.shape[1]), c_i(degree))
    return leaf_rows


def octree_neighbors(node_index: torch.Tensor, leaf_index: torch.Tensor) -> torch.Tensor:
    """K20a.  Sorted int64 id arrays -> (L,6) int32: per leaf and direction (-x, +x, -y, +y, -z, +z)
    the number of the leaf of equal size or coarser across that face, -1 for the cube's boundary,
    empty space or finer leaves (which hold the adjacency from their side)."""
    _want("octree_neighbors", "node_index", node_index, (None,), torch.int64)
    _want("octree_neighbors", "leaf_index", leaf_index, (None,), torch.int64)
    leaves = leaf_index.numel()
    out = torch.empty((leaves, 6), dtype=torch.int32, device=leaf_index.device)
    if leaves > 0:
        _call("ffn_octree_neighbors",
              _dev(node_index if node_index.numel() else None, torch.int64, "node_index"),
              c_i64(node_index.numel()), _dev(leaf_index, torch.int64, "leaf_index"),
              c_i64(leaves), _dev(out, torch.int32))
    return out


TV_CHUNK = 16


class OctreeTVPlan:
    """What K20b / K20c read of a tree's face adjacency, on the device (include/ffn_hip.h, K20):
    ``edge_i`` / ``edge_j`` (E,), the 2 E incidences stably sorted by leaf (``inc_leaf``,
    ``inc_code = 2 edge + [the leaf is the edge's j]``), every leaf's range ``seg_lo`` / ``seg_hi``
    in that order, ``seg_base`` and ``longest``, the longest incidence list.  Made once per tree by
    ``octree_tv_plan``; the workspace of the per-step kernels is kept here between calls."""

    def __init__(self, num_leaves, edge_i, edge_j, inc_leaf, inc_code, seg_lo, seg_hi, seg_base,
                 longest):
        self.num_leaves, self.num_edges = int(num_leaves), int(edge_i.numel())
        self.longest = int(longest)
        self.edge_i, self.edge_j = edge_i, edge_j
        self.inc_leaf, self.inc_code = inc_leaf, inc_code
        self.seg_lo, self.seg_hi, self.seg_base = seg_lo, seg_hi, seg_base
        self.device = seg_lo.device
        self._workspace = {}

    def workspace(self, stride: int) -> Optional[torch.Tensor]:
        if self.num_edges == 0:
            return None
        if stride not in self._workspace:
            need = octree_tv_workspace_bytes(self.num_leaves, self.num_edges, stride)
            self._workspace[stride] = torch.empty(((need + 3) // 4,), dtype=torch.float32,
                                                  device=self.device)
        return self._workspace[stride]


def octree_tv_plan(neighbors: torch.Tensor, leaf_index: torch.Tensor) -> OctreeTVPlan:
    """The plan of K20b / K20c from the (L,6) table of ``octree_neighbors`` and the sorted leaf ids:
    index plumbing on the device (``torch.nonzero``, one stable sort, two cumulative sums), once per
    tree; it reads the edge count and the longest incidence list back.  ``(i, dir)`` is an edge when
    ``j = neighbors[i, dir] >= 0`` and ``level(j) < level(i)`` or ``dir`` is a + direction; edges are
    numbered in ``(i, dir)`` order.  More than ``6 L`` edges or ``2 E >= 2^31`` are refused."""
    leaves = leaf_index.numel()
    if neighbors.dim() != 2 or tuple(neighbors.shape) != (leaves, 6) or neighbors.dtype != torch.int32:
        raise ValueError("octree tv_plan: neighbors must be (num_leaves, 6) int32, got %s %s for %d "
                         "leaves" % (tuple(neighbors.shape), neighbors.dtype, leaves))
    if leaves < 1:
        raise ValueError("octree tv_plan: a tree needs at least one leaf")
    dev = leaf_index.device
    _, levels = octree_leaf_geometry(leaf_index, 1.0)
    nb = neighbors.to(torch.int64)
    other = levels[nb.clamp(min=0)]
    plus = torch.tensor([False, True] * 3, device=dev)
    mask = (nb >= 0) & ((other < levels[:, None]) | plus[None, :])
    at = torch.nonzero(mask.reshape(-1)).reshape(-1)              # (i, dir) order
    edge_i = (at // 6).to(torch.int32)
    edge_j = nb.reshape(-1)[at].to(torch.int32)
    edges = int(at.numel())
    if edges > 6 * leaves or 2 * edges >= 2 ** 31:     # the incidence numbers 2 e + 1 are int32
        raise ValueError("octree tv_plan: %d edges for %d leaves; E <= 6 L and 2 E < 2^31"
                         % (edges, leaves))
    code = torch.arange(2 * edges, dtype=torch.int32, device=dev)
    leaf = torch.stack([edge_i, edge_j], 1).reshape(-1)
    inc_leaf, order = torch.sort(leaf, stable=True)
    inc_code = code[order]
    counts = torch.bincount(inc_leaf.to(torch.int64), minlength=leaves)
    seg_hi = torch.cumsum(counts, 0)
    seg_lo = seg_hi - counts
    before = torch.cumsum((counts > 0).to(torch.int64), 0) - (counts > 0).to(torch.int64)
    seg_base = seg_lo // TV_CHUNK + before
    longest = int(counts.max().item())
    return OctreeTVPlan(leaves, edge_i.contiguous(), edge_j.contiguous(),
                        inc_leaf.to(torch.int32).contiguous(), inc_code.contiguous(),
                        seg_lo.to(torch.int32), seg_hi.to(torch.int32), seg_base.to(torch.int32),
                        longest)


def octree_tv_workspace_bytes(num_leaves: int, num_edges: int, stride: int) -> int:
    """Bytes of workspace ``octree_tv`` needs."""
    fn = _lib.load().ffn_octree_tv_workspace_bytes
    fn.restype = ctypes.c_int64
    size = fn(c_i64(num_leaves), c_i64(num_edges), c_i(stride))
    if size < 0:
        raise _lib.FfnError("ffn_octree_tv_workspace_bytes failed: %s"
                            % _lib.load().ffn_last_error_string().decode())
    return int(size)


def octree_tv_weights(weights, stride: int, degree: Optional[int] = None) -> np.ndarray:
    """The per-column weight vector of K20b, float32 (stride,), padding 0.  A plain tree (``degree``
    None, stride 4, ``[r, g, b, sigma]``): ``weights = (rgb, sigma)``.  An SH tree in the device
    layout ``[sigma, k_r.., k_g.., k_b.., 0 ..]``: ``weights = (band0, higher_bands, sigma)``.
    ``None`` is all ones.  Needs no GPU."""
    count = 2 if degree is None else 3
    if weights is None:
        weights = (1.0,) * count
    try:
        values = [float(w) for w in weights]
    except TypeError:
        raise ValueError("octree tv: weights must be %d numbers, got %r" % (count, weights))
    if len(values) != count:
        raise ValueError("octree tv: weights must be %d numbers (%s), got %r"
                         % (count, "rgb, sigma" if degree is None else "band0, higher_bands, sigma",
                            weights))
    if not all(0.0 <= v < float("inf") for v in values):       # NaN fails too
        raise ValueError("octree tv: weights must be finite and >= 0, got %r" % (weights,))
    out = np.zeros((stride,), np.float32)
    if degree is None:
        if stride != 4:
            raise ValueError("octree tv: a plain tree has rows of 4 floats, got stride %d" % stride)
        out[:3], out[3] = values[0], values[1]
        return out
    channels = octree_sh_channels(degree)
    bases = (channels - 1) // 3
    if stride < channels or stride % 4 != 0:
        raise ValueError("octree tv: stride must be a multiple of 4 and >= %d for degree %d, got %d"
                         % (channels, degree, stride))
    out[0] = values[2]
    for c in range(3):
        out[1 + c * bases] = values[0]
        out[2 + c * bases:1 + (c + 1) * bases] = values[1]
    return out


def octree_tv_check_eps(eps) -> float:
    """``eps`` as a float; ValueError unless it is a positive finite number.  Needs no GPU."""
    eps = float(eps)
    if not 0.0 < eps < float("inf"):                           # NaN fails too
        raise ValueError("octree tv: eps must be positive and finite, got %r" % (eps,))
    return eps


def octree_tv(rows: torch.Tensor, plan: OctreeTVPlan, weights, eps: float,
              d_rows: Optional[torch.Tensor] = None, accumulate: bool = False,
              want_grad: bool = True):
    """K20b + K20c.  rows (L, stride) float32, stride a multiple of 4; ``weights`` a (stride,) vector
    of per-column weights (``octree_tv_weights``), finite and >= 0; -> (value, d_rows): the
    Charbonnier energy ``(1/E) sum_e sum_c w_c (sqrt(d^2 + eps^2) - eps)`` over the plan's edges as a
    device scalar, and its gradient (L, stride), every row written (``accumulate``: added to the
    content of the ``d_rows`` passed in).  Deterministic, no float atomics, no host sync.  No
    geometric weight: every face counts the same whatever its area or the distance of the
    centres.  ``want_grad=False`` (and no ``d_rows``) computes the value alone: the entry point gets a
    null ``d_rows``, skips the reduction and ``(value, None)`` comes back."""
    if not isinstance(plan, OctreeTVPlan):
        raise TypeError("octree tv: plan must be an OctreeTVPlan (ops.octree_tv_plan)")
    eps = octree_tv_check_eps(eps)
    _want_tensors("octree tv", rows=rows)
    if rows.dim() != 2 or rows.shape[1] % 4 != 0 or not 4 <= rows.shape[1] <= 64:
        raise ValueError("octree tv: rows must be (num_leaves, stride) with stride a multiple of 4 "
                         "in 4 .. 64, got %s" % (tuple(rows.shape),))
    leaves, stride = rows.shape
    if leaves != plan.num_leaves:
        raise ValueError("octree tv: the plan is of a tree with %d leaves, rows has %d"
                         % (plan.num_leaves, leaves))
    lam = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    if len(lam) != stride:
        raise ValueError("octree tv: %d weights for rows of %d floats" % (len(lam), stride))
    if not (np.isfinite(lam).all() and (lam >= 0).all()):
        raise ValueError("octree tv: weights must be finite and >= 0, got %r" % (lam.tolist(),))
    if rows.data_ptr() % 16 != 0:
        raise ValueError("octree tv: rows must be 16-byte aligned")
    if accumulate and d_rows is None:
        raise ValueError("octree tv: accumulate needs the d_rows to add to")
    if not want_grad and d_rows is not None:
        raise ValueError("octree tv: want_grad=False takes no d_rows")
    if d_rows is None and want_grad:
        d_rows = torch.empty_like(rows)
    if d_rows is not None and d_rows.shape != rows.shape:
        raise ValueError("octree tv: d_rows must be %s, got %s" % (tuple(rows.shape),
                                                                   tuple(d_rows.shape)))
    if d_rows is not None and d_rows.data_ptr() % 16 != 0:
        raise ValueError("octree tv: d_rows must be 16-byte aligned")
    value = torch.empty((), dtype=torch.float32, device=rows.device)
    workspace = plan.workspace(stride)
    host = (ctypes.c_float * stride)(*[float(v) for v in lam])
    _call("ffn_octree_tv", _dev(rows, name="rows"), c_i64(leaves), c_i(stride),
          _dev(plan.edge_i, torch.int32), _dev(plan.edge_j, torch.int32), c_i64(plan.num_edges),
          _dev(plan.inc_leaf, torch.int32), _dev(plan.inc_code, torch.int32),
          _dev(plan.seg_lo, torch.int32), _dev(plan.seg_hi, torch.int32),
          _dev(plan.seg_base, torch.int32), c_i64(plan.longest), host, c_f(eps), _dev(value),
          _dev(d_rows, name="d_rows"), c_i(1 if accumulate else 0), _dev(workspace),
          c_i64(0 if workspace is None else workspace.numel() * 4))
    return value, d_rows


def octree_bake(logits: torch.Tensor) -> torch.Tensor:
    """Raw model logits (L,4) [r, g, b, sigma] -> (L,4) float32 [sigmoid(r), sigmoid(g),
    sigmoid(b), softplus(sigma)], the activations of the compositing kernels bit for bit."""
    _want_tensors("octree bake", logits=logits)
    if logits.dim() != 2 or logits.shape[1] != 4:
        raise ValueError("octree bake: logits must be (L,4), got %s" % (tuple(logits.shape),))
    out = torch.empty_like(logits)
    if logits.shape[0] > 0:
        _call("ffn_octree_bake", _dev(logits, name="logits"), c_i64(logits.shape[0]), _dev(out))
    return out


def octree_cell_centers(first_code: int, count: int, center, scale: float, depth: int,
                        device) -> torch.Tensor:
    """K16a.  -> (count,3) float32 on ``device``: the centres of the finest cells (level
    ``depth - 1``) with the path codes ``first_code .. first_code + count - 1``, shifted by the
    cube's ``center``."""
    _want_int("octree_cell_centers", "depth", depth, 1, octree_max_depth())
    _want_int("octree_cell_centers", "count", count, 0, 8 ** (depth - 1))
    _want_int("octree_cell_centers", "first_code", first_code, 0, 8 ** (depth - 1) - count)
    out = torch.empty((count, 3), dtype=torch.float32, device=device)
    _call("ffn_octree_cell_centers", c_i64(first_code), c_i64(count), c_f(center[0]),
          c_f(center[1]), c_f(center[2]), c_f(scale), c_i(depth), _dev(out))
    return out


def octree_density_select(logits: torch.Tensor, first_code: int, tau: float, side: float,
                          depth: int):
    """K16b.  logits (N,4) of the cells ``first_code .. first_code + N - 1`` -> codes (K) int32 and
    data (K,4) float32 of the cells with ``softplus(sigma) * side > tau``, in code order; data is
    what ``octree_bake`` makes of the kept rows.  Reads the count back once."""
    _want_tensors("octree density select", logits=logits)
    _want_int("octree density select", "depth", depth, 1, octree_max_depth())
    if logits.dim() != 2 or logits.shape[1] != 4:
        raise ValueError("octree density select: logits must be (N,4), got %s"
                         % (tuple(logits.shape),))
    n = logits.shape[0]
    dev = logits.device
    activated = torch.empty((n, 4), dtype=torch.float32, device=dev)
    codes = torch.empty((n,), dtype=torch.int32, device=dev)
    data = torch.empty((n, 4), dtype=torch.float32, device=dev)
    total = torch.zeros((), dtype=torch.int32, device=dev)
    flags, offsets, tiles = _scan_scratch(n, dev)
    _call("ffn_octree_density_select", _dev(logits, name="logits"), c_i64(first_code), c_i64(n),
          c_f(tau), c_f(side), c_i(depth), _dev(flags, torch.uint8), _dev(offsets, torch.int32),
          _dev(tiles, torch.int32), _dev(activated), _dev(codes, torch.int32), _dev(data),
          _dev(total, torch.int32))
    k = int(total.item())
    return codes[:k].clone(), data[:k].clone()


def octree_merge_level(codes: torch.Tensor, levels: torch.Tensor, data: torch.Tensor, level: int,
                       depth: int, rgb_tol: float, sigma_tol: float):
    """K16c.  One coarsening pass over the code-sorted leaf list (codes (N) int32 left-aligned to
    the finest level, levels (N) int32, data (N,4) float32): eight sibling leaves of ``level``
    within the tolerances of their mean become their parent.  -> the new (codes, levels, data).
    Reads the count back once."""
    _want_tensors("octree merge level", codes=codes, levels=levels, data=data)
    _want_int("octree merge level", "depth", depth, 2, octree_max_depth())
    _want_int("octree merge level", "level", level, 1, depth - 1)
    n = codes.shape[0]
    dev = codes.device
    if levels.shape != (n,) or data.shape != (n, 4):
        raise ValueError("octree merge level: codes (N), levels (N) and data (N,4) disagree")
    merge = torch.empty((n,), dtype=torch.uint8, device=dev)
    codes_out, levels_out, data_out = (torch.empty_like(codes), torch.empty_like(levels),
                                       torch.empty_like(data))
    total = torch.zeros((), dtype=torch.int32, device=dev)
    flags, offsets, tiles = _scan_scratch(n, dev)
    _call("ffn_octree_merge_level", _dev(codes, torch.int32, "codes"),
          _dev(levels, torch.int32, "levels"), _dev(data, name="data"), c_i64(n), c_i(level),
          c_i(depth), c_f(rgb_tol), c_f(sigma_tol), _dev(merge, torch.uint8),
          _dev(flags, torch.uint8), _dev(offsets, torch.int32), _dev(tiles, torch.int32),
          _dev(codes_out, torch.int32), _dev(levels_out, torch.int32), _dev(data_out),
          _dev(total, torch.int32))
    k = int(total.item())
    return codes_out[:k].clone(), levels_out[:k].clone(), data_out[:k].clone()


# --------------------------------------------------------------------------------- K21
def octree_leaf_weights(starts: torch.Tensor, directions: torch.Tensor, scale: float, depth: int,
                        node_index: torch.Tensor, leaf_index: torch.Tensor, rows: torch.Tensor,
                        stride: int, sigma_offset: int, t_min: float = 0.0,
                        min_transmittance: float = 0.0,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K21a.  Per leaf the largest compositing weight ``w = T * a`` that any of the rays gives it on
    the walk of ``octree_render_volume`` -> (L,) float32.  ``rows`` (L, stride) float32 of which only
    the density ``rows[:, sigma_offset]`` is read: stride 4 and offset 3 for ``[r, g, b, sigma]``,
    the stride of ``octree_sh_device_layout`` and offset 0 for SH rows.  With ``out`` (L,) float32
    given the maxima fold into it (and it is returned): cameras or chunks of rays, in any order,
    give the bits of one call over all of them.  ``out`` holds weights, that is values >= 0."""
    _walk_check(starts, directions, scale, depth, node_index, leaf_index)
    _want_tensors("octree leaf_weights", rows=rows)
    stride, sigma_offset = int(stride), int(sigma_offset)
    if (rows.dim() != 2 or rows.shape[0] != leaf_index.numel() or rows.shape[1] != stride
            or stride < 1 or not 0 <= sigma_offset < stride):
        raise ValueError("octree leaf_weights: rows must be (num_leaves, stride) with 0 <= "
                         "sigma_offset < stride, got %s for %d leaves, stride %d, sigma_offset %d"
                         % (tuple(rows.shape), leaf_index.numel(), stride, sigma_offset))
    _check_min_transmittance("octree leaf_weights", min_transmittance)
    if out is None:
        out = torch.zeros((leaf_index.numel(),), dtype=torch.float32, device=starts.device)
    elif out.shape != (leaf_index.numel(),):
        raise ValueError("octree leaf_weights: out must be (num_leaves,) = (%d,), got %s"
                         % (leaf_index.numel(), tuple(out.shape)))
    if starts.shape[0] > 0:
        _call("ffn_octree_leaf_weights", *_walk_args(starts, directions, scale, depth, node_index,
                                                     leaf_index),
              c_f(t_min), _dev(rows, name="rows"), c_i(stride), c_i(sigma_offset),
              c_f(min_transmittance), _dev(out, name="out"))
    return out


# --------------------------------------------------------------------------------- K29
def octree_distortion(starts: torch.Tensor, directions: torch.Tensor, scale: float, depth: int,
                      node_index: torch.Tensor, leaf_index: torch.Tensor, rows: torch.Tensor,
                      stride: int, sigma_offset: int, t_min: float = 0.0,
                      min_transmittance: float = 0.0) -> torch.Tensor:
    """K29a.  Per ray the distortion ``D = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 L_i`` of
    the weights ``w = T * a`` that ``octree_render_volume`` composites with, over the leaves it takes:
    ``m`` a chord's midpoint and ``L`` its length, both as world lengths along the ray -> (N,)
    float32, +0 for a ray that takes no leaf.  ``rows``, ``stride`` and ``sigma_offset`` as for
    ``octree_leaf_weights`` (only the density is read).  No atomics: the same bits on every call."""
    _walk_check(starts, directions, scale, depth, node_index, leaf_index)
    _want_tensors("octree distortion", rows=rows)
    stride, sigma_offset = int(stride), int(sigma_offset)
    if (rows.dim() != 2 or rows.shape[0] != leaf_index.numel() or rows.shape[1] != stride
            or stride < 1 or not 0 <= sigma_offset < stride):
        raise ValueError("octree distortion: rows must be (num_leaves, stride) with 0 <= "
                         "sigma_offset < stride, got %s for %d leaves, stride %d, sigma_offset %d"
                         % (tuple(rows.shape), leaf_index.numel(), stride, sigma_offset))
    _check_min_transmittance("octree distortion", min_transmittance)
    out = torch.zeros((starts.shape[0],), dtype=torch.float32, device=starts.device)
    if starts.shape[0] > 0:
        _call("ffn_octree_distortion", *_walk_args(starts, directions, scale, depth, node_index,
                                                   leaf_index),
              c_f(t_min), _dev(rows, name="rows"), c_i(stride), c_i(sigma_offset),
              c_f(min_transmittance), _dev(out, name="out"))
    return out


# --------------------------------------------------------------------------------- K26
def octree_focus_sample(starts: torch.Tensor, directions: torch.Tensor, near_far: torch.Tensor,
                        ray_index: torch.Tensor, center, scale: float, depth: int,
                        node_index: torch.Tensor, leaf_index: torch.Tensor, rows: torch.Tensor,
                        stride: int, sigma_offset: int, u: torch.Tensor,
                        t_uniform: Optional[torch.Tensor] = None,
                        n_uniform: Optional[int] = None, min_mass: float = 1e-3,
                        want_mass: bool = False):
    """K26.  Focus samples of the rays ``ray_index`` (R,) int64 drawn from the tree's own compositing
    weights along each ray, merged with the rays' uniform samples -> t (R, n_uniform + n_focus)
    float32, every row ascending; with ``want_mass`` also the weight sum M (R,) of every ray.
    starts, directions (N,3) and near_far (2,N) are the sampler's per-ray state in WORLD coordinates
    (``center``, three floats, is subtracted from the starts inside the kernel).  ``rows`` / ``stride``
    / ``sigma_offset`` as for ``octree_leaf_weights``.  ``u`` (R, n_focus) in [0,1], ascending in
    every row.  ``t_uniform`` (R, >= n_uniform): the first ``n_uniform`` columns of a row are its
    ascending uniform samples (default: all its columns); None gives the focus samples alone.  A ray
    whose M is not positive or below ``min_mass``, that misses the cube or has no near < far gets
    ``near + u * (far - near)``."""
    who = "octree focus_sample"
    _want_tensors(who, starts=starts, directions=directions, near_far=near_far,
                  ray_index=ray_index, leaf_index=leaf_index, rows=rows, u=u)
    _want(who, "node_index", node_index, (None,), torch.int64)
    _want_int(who, "depth", depth, 1, 11)
    n = starts.shape[0]
    if starts.shape != (n, 3) or directions.shape != (n, 3) or near_far.shape != (2, n):
        raise ValueError("%s: starts and directions must be (N,3) and near_far (2,N)" % who)
    rays = ray_index.shape[0]
    if ray_index.dim() != 1 or u.dim() != 2 or u.shape[0] != rays:
        raise ValueError("%s: ray_index must be (R,) and u (R, n_focus)" % who)
    n_focus = int(u.shape[1])
    if n_focus < 1:
        raise ValueError("%s: n_focus >= 1" % who)
    stride, sigma_offset = int(stride), int(sigma_offset)
    if (rows.dim() != 2 or rows.shape[0] != leaf_index.numel() or rows.shape[1] != stride
            or stride < 1 or not 0 <= sigma_offset < stride):
        raise ValueError("%s: rows must be (num_leaves, stride) with 0 <= sigma_offset < stride, "
                         "got %s for %d leaves, stride %d, sigma_offset %d"
                         % (who, tuple(rows.shape), leaf_index.numel(), stride, sigma_offset))
    if not float(min_mass) >= 0.0:       # NaN fails too
        raise ValueError("%s: min_mass must be >= 0, got %r" % (who, min_mass))
    if t_uniform is None:
        if n_uniform not in (None, 0):
            raise ValueError("%s: n_uniform = %d without t_uniform" % (who, n_uniform))
        n_uniform, uniform_stride = 0, 0
    else:
        if t_uniform.dim() != 2 or t_uniform.shape[0] != rays:
            raise ValueError("%s: t_uniform must be (R, >= n_uniform)" % who)
        uniform_stride = int(t_uniform.shape[1])
        n_uniform = uniform_stride if n_uniform is None else int(n_uniform)
        if not 0 <= n_uniform <= uniform_stride:
            raise ValueError("%s: 0 <= n_uniform <= t_uniform.shape[1]" % who)
    if rays * (n_uniform + n_focus) >= 1 << 31:
        raise ValueError("%s: R * (n_uniform + n_focus) must stay below 2^31" % who)
    ptrs = (_dev(starts, name="starts"), _dev(directions, name="directions"),
            _dev(near_far, name="near_far"), _dev(ray_index, torch.int64, "ray_index"),
            _dev(node_index if node_index.numel() else None, torch.int64, "node_index"),
            _dev(leaf_index, torch.int64, "leaf_index"), _dev(rows, name="rows"), _dev(u, name="u"),
            _dev(t_uniform if n_uniform else None, name="t_uniform"))
    t = torch.empty((rays, n_uniform + n_focus), dtype=torch.float32, device=starts.device)
    mass = torch.empty((rays,), dtype=torch.float32, device=starts.device) if want_mass else None
    if rays > 0:
        cx, cy, cz = (float(c) for c in center)
        _call("ffn_octree_focus_sample", ptrs[0], ptrs[1], ptrs[2], c_i64(n), ptrs[3], c_i(rays),
              c_f(cx), c_f(cy), c_f(cz), c_f(scale), c_i(depth), ptrs[4],
              c_i64(node_index.numel()), ptrs[5], c_i64(leaf_index.numel()), ptrs[6], c_i(stride),
              c_i(sigma_offset), ptrs[7], c_i(n_focus), ptrs[8], c_i(uniform_stride),
              c_i(n_uniform), c_f(min_mass), _dev(t, name="t_out"), _dev(mass, name="mass_out"))
    return (t, mass) if want_mass else t


OCTREE_DROP, OCTREE_KEEP, OCTREE_SPLIT = 0, 1, 2


def octree_max_points() -> int:
    """The most elements one K12 flag scan holds (a host function of the library: no GPU needed)."""
    fn = _lib.load().ffn_octree_max_points
    fn.restype = ctypes.c_int64
    return int(fn())


def octree_refine_check_action(action, num_leaves: int) -> None:
    """The refusals of ``octree_refine`` that need no device: ``action`` (numpy or tensor) is
    one-dimensional, of the tree's leaf count, and 8 of its slots per leaf fit one scan."""
    if action.ndim != 1 or action.shape[0] != num_leaves:
        raise ValueError("octree refine: action must be (num_leaves,) = (%d,), got %s"
                         % (num_leaves, tuple(action.shape)))
    if 8 * num_leaves > octree_max_points():
        raise ValueError("octree refine: %d leaves could become %d, a new leaf count at or over "
                         "the limit of 2^31" % (num_leaves, 8 * num_leaves))


def _octree_refine_count(action_c: torch.Tensor):
    """K21b's first launch on the actions in code order -> (flags, offsets, total): the scan of the
    8 L slots and, as a device scalar, the new leaf count.  No read-back."""
    num, dev = action_c.shape[0], action_c.device
    flags, offsets, tiles = _scan_scratch(8 * num, dev)
    total = torch.zeros((), dtype=torch.int32, device=dev)
    _call("ffn_octree_refine_count", _dev(action_c, torch.uint8, "action"), c_i64(num),
          _dev(flags, torch.uint8), _dev(offsets, torch.int32), _dev(tiles, torch.int32),
          _dev(total, torch.int32))
    return flags, offsets, total


def _octree_refine_scatter(action_c, flags, offsets, ids_c, rows_c, with_rows: bool, channels: int,
                           count: int):
    """K21b's second launch for the ``count`` new leaves of ``_octree_refine_count``'s scan, all
    arrays in code order -> (new_ids, new_rows or None, parent).  No read-back."""
    num, dev = ids_c.shape[0], ids_c.device
    new_ids = torch.empty((count,), dtype=torch.int64, device=dev)
    parent = torch.empty((count,), dtype=torch.int32, device=dev)
    new_rows = torch.empty((count, channels), dtype=torch.float32, device=dev) if with_rows else None
    _call("ffn_octree_refine_scatter", _dev(action_c, torch.uint8, "action"),
          _dev(flags, torch.uint8), _dev(offsets, torch.int32), _dev(ids_c, torch.int64, "leaf_ids"),
          _dev(rows_c, name="rows"), c_i64(num), c_i(channels), c_i64(count),
          _dev(new_ids, torch.int64), _dev(new_rows if channels else None), _dev(parent, torch.int32))
    return new_ids, new_rows, parent


def octree_refine(leaf_ids: torch.Tensor, rows: Optional[torch.Tensor], action: torch.Tensor,
                  depth: int):
    """K21b.  ``leaf_ids`` (L,) int64 sorted (a tree's ``leaf_index``), ``rows`` (L,C) float32 or
    None, ``action`` (L,) uint8: 0 drop, 1 keep, 2 split into the eight children, which inherit the
    row bit for bit.  ``depth`` is the tree's (1 + its deepest level); a leaf id deeper than that is
    refused.  -> ``(leaf_ids, node_ids, rows, parent)`` of the new tree, sorted by id; ``parent``
    (L',) int64 is the number of the old leaf a new one came from.  Raises ``ValueError`` for an
    action of the wrong length or with a value above 2, when no leaf is left, when a split leaf sits
    at level ``octree_max_depth() - 1`` (the tree would pass the ray walk's depth limit of 11) and
    when the new leaf count could reach 2^31.  Reads one small block of counts back; the sort to code
    order and back to id order, the interior nodes (K12h) and the permutations are plumbing."""
    _want_tensors("octree refine", leaf_ids=leaf_ids, action=action)
    num = leaf_ids.shape[0]
    dev = leaf_ids.device
    depth = int(depth)
    limit = octree_max_depth()
    if num < 1 or depth < 1 or depth > limit:
        raise ValueError("octree refine: at least one leaf and 1 <= depth <= %d, got %d leaves, "
                         "depth %d" % (limit, num, depth))
    octree_refine_check_action(action, num)
    if rows is not None and (rows.dim() != 2 or rows.shape[0] != num):
        raise ValueError("octree refine: rows must be (num_leaves, C) = (%d, C), got %s"
                         % (num, tuple(rows.shape)))
    channels = 0 if rows is None else int(rows.shape[1])
    # (code, level) from the ids: integer plumbing, as in build_from_model
    first_id = torch.tensor([(8 ** k - 1) // 7 for k in range(limit + 1)], dtype=torch.int64,
                            device=dev)
    levels = torch.searchsorted(first_id, leaf_ids, right=True) - 1
    codes = (leaf_ids - first_id[levels]) << (3 * (limit - 1 - levels).clamp(min=0))
    codes, order = torch.sort(codes)                   # id order -> code order
    ids_c = leaf_ids[order].contiguous()
    action_c = action[order].contiguous()
    rows_c = None if rows is None or channels == 0 else rows[order].contiguous()
    # the scan runs before the action's values and the levels are judged, so that the new count and
    # what the refusals need come back in ONE read-back; a value above 2 sets no flag in the kernel
    flags, offsets, total = _octree_refine_count(action_c)
    split = action == OCTREE_SPLIT
    stats = torch.stack([total.to(torch.int64), action.max().to(torch.int64), levels.max(),
                         torch.where(split, levels, -1).max(),
                         torch.where(action == OCTREE_DROP, -1, levels).max()]).cpu().tolist()
    count, top_action, top_level, top_split, top_kept = [int(v) for v in stats]
    if top_action > OCTREE_SPLIT:
        raise ValueError("octree refine: an action is 0 (drop), 1 (keep) or 2 (split), got %d"
                         % top_action)
    if top_level > depth - 1:
        raise ValueError("octree refine: a leaf at level %d in a tree of depth %d"
                         % (top_level, depth))
    if top_split >= limit - 1:
        raise ValueError("octree refine: a leaf at level %d cannot split: the tree would be deeper "
                         "than the ray walk's limit of %d (octree_max_depth())"
                         % (top_split, limit))
    if count < 1:
        raise ValueError("octree refine: the action leaves no leaf; a tree needs at least one")
    new_ids, new_rows, parent = _octree_refine_scatter(action_c, flags, offsets, ids_c, rows_c,
                                                       rows is not None, channels, count)
    new_depth = max(top_kept, top_split + 1) + 1
    node_ids = octree_interior_nodes(new_ids, new_depth)      # wants code order
    new_ids, back = torch.sort(new_ids)                       # code order -> id order
    parent = order[parent.to(torch.int64)[back]]
    if new_rows is not None:
        new_rows = new_rows[back].contiguous()
    return new_ids, torch.sort(node_ids)[0], new_rows, parent


# --------------------------------------------------------------------------------- K22
MESH_MAX_PER_TRIANGLE = 1 << 24     # the reference's f32 van der Corput digits hold below this
MESH_MAX_TEXTURE_SIDE = 1 << 24     # a row or column index is exact in f32


def mesh_sample_check(vertices, triangles, uvs, offsets, texture) -> int:
    """The refusals of ``mesh_sample``, none of which needs a device: shapes, dtypes, vertex ids,
    finite UVs, the prefix sum and its limits.  Tensors on any device (the small ones are read
    back).  -> N, the number of samples.  Raises ``ValueError`` naming the argument."""
    def want(name, t, dtype, shape):
        if not torch.is_tensor(t) or t.dtype != dtype:
            raise ValueError("mesh_sample: %s must be a %s tensor, got %s"
                             % (name, dtype, t.dtype if torch.is_tensor(t) else type(t).__name__))
        if t.dim() != len(shape) or any(w is not None and w != g for w, g in zip(shape, t.shape)):
            raise ValueError("mesh_sample: %s must be (%s), got %s"
                             % (name, ", ".join("*" if w is None else str(w) for w in shape),
                                tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("mesh_sample: %s must be contiguous" % name)

    want("vertices", vertices, torch.float32, (None, 3))
    num_vertices = vertices.shape[0]
    want("triangles", triangles, torch.int32, (None, 3))
    num_triangles = triangles.shape[0]
    want("uvs", uvs, torch.float32, (num_vertices, 2))
    want("offsets", offsets, torch.int32, (num_triangles + 1,))
    want("texture", texture, torch.uint8, (None, None, None))
    if num_vertices < 1 or num_vertices > (2 ** 31 - 1) // 3:
        raise ValueError("mesh_sample: vertices holds %d vertices; 1 .. (2^31 - 1) / 3 are "
                         "supported" % num_vertices)
    if num_triangles < 1 or num_triangles > (2 ** 31 - 1) // 3:
        raise ValueError("mesh_sample: triangles holds %d triangles; 1 .. (2^31 - 1) / 3 are "
                         "supported" % num_triangles)
    height, width, channels = texture.shape
    if (channels < 3 or not 1 <= height <= MESH_MAX_TEXTURE_SIDE
            or not 1 <= width <= MESH_MAX_TEXTURE_SIDE or height * width * channels >= 2 ** 31):
        raise ValueError("mesh_sample: texture must be (H, W, C) with C >= 3, 1 <= H, W <= 2^24 "
                         "and fewer than 2^31 bytes, got %s" % (tuple(texture.shape),))
    low, high = [int(v) for v in torch.stack([triangles.min(), triangles.max()]).cpu()]
    if low < 0 or high >= num_vertices:
        raise ValueError("mesh_sample: triangles indexes vertices %d .. %d, outside 0 .. %d"
                         % (low, high, num_vertices - 1))
    if not bool(torch.isfinite(uvs).all()):
        raise ValueError("mesh_sample: uvs holds a NaN or an infinity")
    steps = offsets.cpu().numpy().astype(np.int64)
    counts = np.diff(steps)
    if steps[0] != 0 or (counts < 0).any():
        raise ValueError("mesh_sample: offsets must start at 0 and never decrease (the exclusive "
                         "prefix sum of the per-triangle counts)")
    if counts.max() >= MESH_MAX_PER_TRIANGLE:
        raise ValueError("mesh_sample: offsets gives one triangle %d samples; fewer than 2^24 per "
                         "triangle are supported" % counts.max())
    total = int(steps[-1])
    if total < 1 or total > octree_max_points():
        raise ValueError("mesh_sample: offsets ends at N = %d samples; 1 .. %d are supported"
                         % (total, octree_max_points()))
    return total


def mesh_sample(vertices: torch.Tensor, triangles: torch.Tensor, uvs: torch.Tensor,
                offsets: torch.Tensor, texture: torch.Tensor, want_uvs: bool = False):
    """K22.  Surface samples of a textured mesh.  vertices (V,3) f32 (already normalised), triangles
    (F,3) int32, uvs (V,2) f32, offsets (F+1,) int32 (the exclusive prefix sum of the per-triangle
    sample counts, ``offsets[F] = N``), texture (H,W,C) uint8 with C >= 3 and the row index growing
    with ``v`` -> positions (N,3), colors (N,3) float32 [, sample_uvs (N,2)].  Sample ``k`` of a
    triangle is the Basu-Owen point ``k + 1``; the same inputs give the same bits.  Bad input is a
    ``ValueError`` (``mesh_sample_check``: the ids, the UVs and the offsets are read back once)."""
    n = mesh_sample_check(vertices, triangles, uvs, offsets, texture)
    return _mesh_sample_launch(vertices, triangles, uvs, offsets, texture, n, want_uvs)


def _mesh_sample_launch(vertices, triangles, uvs, offsets, texture, n: int, want_uvs: bool):
    """The launch of ``mesh_sample`` for ``n = offsets[F]`` samples of checked arguments: the
    outputs and the call, no read-back."""
    dev = vertices.device
    positions = torch.empty((n, 3), dtype=torch.float32, device=dev)
    colors = torch.empty((n, 3), dtype=torch.float32, device=dev)
    sample_uvs = torch.empty((n, 2), dtype=torch.float32, device=dev) if want_uvs else None
    height, width, channels = texture.shape
    _call("ffn_mesh_sample", _dev(vertices, name="vertices"), c_i64(vertices.shape[0]),
          _dev(triangles, torch.int32, "triangles"), c_i64(triangles.shape[0]),
          _dev(uvs, name="uvs"), _dev(offsets, torch.int32, "offsets"), c_i64(n),
          _dev(texture, torch.uint8, "texture"), c_i(height), c_i(width), c_i(channels),
          _dev(positions), _dev(colors), _dev(sample_uvs))
    if want_uvs:
        return positions, colors, sample_uvs
    return positions, colors


# --------------------------------------------------------------------------------- K23
def octree_carve_max_cameras() -> int:
    """The most cameras K23 takes: ``255 * C`` must be exact in f32 (``C <= 2^24 / 255``)."""
    fn = _lib.load().ffn_octree_carve_max_cameras
    fn.restype = ctypes.c_int
    return int(fn())


def octree_carve_check(images_u8, mask_u8, proj, first_code, count, depth, alpha_u8, max_misses,
                       min_views):
    """The refusals of ``octree_carve_select``, none of which needs a device: shapes, dtypes,
    contiguity, 4 channels, ``C >= 1`` and its limit, a finite ``proj`` (read back once), a chunk
    that lies in the grid and fits the scan, and the ranges of the scalars.  Tensors on any device.
    -> (C, H, W).  Raises ``ValueError`` naming the argument."""
    def want(name, t, dtype, shape):
        if not torch.is_tensor(t) or t.dtype != dtype:
            raise ValueError("octree_carve_select: %s must be a %s tensor, got %s"
                             % (name, dtype, t.dtype if torch.is_tensor(t) else type(t).__name__))
        if t.dim() != len(shape) or any(w is not None and w != g for w, g in zip(shape, t.shape)):
            raise ValueError("octree_carve_select: %s must be (%s), got %s"
                             % (name, ", ".join("*" if w is None else str(w) for w in shape),
                                tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("octree_carve_select: %s must be contiguous" % name)

    want("images_u8", images_u8, torch.uint8, (None, None, None, 4))
    cameras, height, width = images_u8.shape[:3]
    want("mask_u8", mask_u8, torch.uint8, (cameras, height, width))
    want("proj", proj, torch.float32, (cameras, 3, 4))
    limit = octree_carve_max_cameras()
    if cameras < 1 or cameras > limit:
        raise ValueError("octree_carve_select: images_u8 holds %d cameras; 1 .. %d are supported "
                         "(255 * C must be exact in f32)" % (cameras, limit))
    if not 1 <= height <= 1 << 24 or not 1 <= width <= 1 << 24:
        raise ValueError("octree_carve_select: images_u8 must be (C, H, W, 4) with 1 <= H, W <= "
                         "2^24, got %s" % (tuple(images_u8.shape),))
    if not bool(torch.isfinite(proj).all()):
        raise ValueError("octree_carve_select: proj holds a NaN or an infinity")
    depth, first_code, count = int(depth), int(first_code), int(count)
    if depth < 1 or depth > octree_max_depth():
        raise ValueError("octree_carve_select: depth %d is outside what the path codes hold "
                         "(1 .. %d)" % (depth, octree_max_depth()))
    if count < 1 or count > octree_max_points():
        raise ValueError("octree_carve_select: count = %d cells in one chunk; 1 .. %d fit the "
                         "scan" % (count, octree_max_points()))
    if first_code < 0 or first_code + count > 8 ** (depth - 1):
        raise ValueError("octree_carve_select: first_code %d and count %d leave the %d cells of "
                         "depth %d" % (first_code, count, 8 ** (depth - 1), depth))
    if not 1 <= int(alpha_u8) <= 255:
        raise ValueError("octree_carve_select: alpha_u8 must lie in 1 .. 255, got %r" % (alpha_u8,))
    if not 0 <= int(max_misses) < 2 ** 31 or not 0 <= int(min_views) < 2 ** 31:
        raise ValueError("octree_carve_select: max_misses and min_views must be >= 0, got %r and "
                         "%r" % (max_misses, min_views))
    return cameras, height, width


def octree_carve_select(images_u8: torch.Tensor, mask_u8: torch.Tensor, proj: torch.Tensor,
                        first_code: int, count: int, center, scale: float, depth: int,
                        alpha_u8: int, max_misses: int, min_views: int, sigma0: float,
                        want_visited: bool = False):
    """K23.  images_u8 (C,H,W,4) uint8 RGBA, mask_u8 (C,H,W) uint8 (0 = background), proj (C,3,4)
    float32 (``cameras.projection_matrices``) -> codes (K) int32 and data (K,4) float32
    ``[r, g, b, sigma0]`` of the cells among ``first_code .. first_code + count - 1`` of the finest
    level whose centre (``octree_cell_centers``) falls on the background in at most ``max_misses``
    of the cameras that see it and that at least ``min_views`` cameras see, in code order.  The
    colour is the mean of the pixels, with own alpha >= ``alpha_u8``, that the centre projects to
    (0.5 when there is none).  Reads the count back once.  With ``want_visited`` also (count,)
    int32: how many cameras each cell's loop looked at.  Bad input is a ``ValueError``
    (``octree_carve_check``)."""
    cameras, height, width = octree_carve_check(images_u8, mask_u8, proj, first_code, count,
                                                depth, alpha_u8, max_misses, min_views)
    n = int(count)
    dev = images_u8.device
    rows = torch.empty((n, 4), dtype=torch.float32, device=dev)
    codes = torch.empty((n,), dtype=torch.int32, device=dev)
    data = torch.empty((n, 4), dtype=torch.float32, device=dev)
    total = torch.zeros((), dtype=torch.int32, device=dev)
    visited = torch.empty((n,), dtype=torch.int32, device=dev) if want_visited else None
    flags, offsets, tiles = _scan_scratch(n, dev)
    _call("ffn_octree_carve_select", _dev(images_u8, torch.uint8, "images_u8"),
          _dev(mask_u8, torch.uint8, "mask_u8"), _dev(proj, name="proj"), c_i(cameras),
          c_i(height), c_i(width), c_i64(int(first_code)), c_i64(n), c_f(center[0]),
          c_f(center[1]), c_f(center[2]), c_f(scale), c_i(int(depth)), c_i(int(alpha_u8)),
          c_i(int(max_misses)), c_i(int(min_views)), c_f(sigma0), _dev(flags, torch.uint8),
          _dev(offsets, torch.int32), _dev(tiles, torch.int32), _dev(rows),
          _dev(visited, torch.int32), _dev(codes, torch.int32), _dev(data),
          _dev(total, torch.int32))
    k = int(total.item())
    if want_visited:
        return codes[:k].clone(), data[:k].clone(), visited
    return codes[:k].clone(), data[:k].clone()


# --------------------------------------------------------------------------------- K27
def octree_carve_box_tables(mask_u8: torch.Tensor) -> torch.Tensor:
    """mask_u8 (C,H,W) uint8 (0 = background) -> the summed-area tables K27 reads, (C,H+1,W+1)
    int32: ``sat[c, r, q]`` = the foreground pixels of camera c in rows ``< r`` and columns ``< q``.
    Two int32 ``torch.cumsum``: exact integers, so ``H * W < 2^31``."""
    if not torch.is_tensor(mask_u8) or mask_u8.dtype != torch.uint8 or mask_u8.dim() != 3:
        raise ValueError("octree_carve_box_level: mask_u8 must be a (C, H, W) torch.uint8 tensor")
    cameras, height, width = mask_u8.shape
    if height * width >= 2 ** 31:
        raise ValueError("octree_carve_box_level: mask_u8 has H * W = %d pixels; fewer than 2^31 "
                         "fit the int32 summed-area table" % (height * width))
    sat = torch.zeros((cameras, height + 1, width + 1), dtype=torch.int32, device=mask_u8.device)
    inner = (mask_u8 != 0).to(torch.int32)
    sat[:, 1:, 1:] = torch.cumsum(torch.cumsum(inner, 1, dtype=torch.int32), 2, dtype=torch.int32)
    return sat


def octree_carve_box_check(images_u8, sat, proj, candidates, expand, level, depth, alpha_u8,
                           max_misses, min_views):
    """The refusals of ``octree_carve_box_level``, none of which needs a device: shapes, dtypes,
    contiguity, the camera limit, ``H * W < 2^31``, a finite ``proj`` (read back once), a level
    inside the tree, a candidate list that fits the scan, and the ranges of the scalars.  Tensors on
    any device.  -> (C, H, W, count).  Raises ``ValueError`` naming the argument."""
    who = "octree_carve_box_level"

    def want(name, t, dtype, shape):
        if not torch.is_tensor(t) or t.dtype != dtype:
            raise ValueError("%s: %s must be a %s tensor, got %s"
                             % (who, name, dtype, t.dtype if torch.is_tensor(t) else type(t).__name__))
        if t.dim() != len(shape) or any(w is not None and w != g for w, g in zip(shape, t.shape)):
            raise ValueError("%s: %s must be (%s), got %s"
                             % (who, name, ", ".join("*" if w is None else str(w) for w in shape),
                                tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (who, name))

    want("images_u8", images_u8, torch.uint8, (None, None, None, 4))
    cameras, height, width = images_u8.shape[:3]
    want("sat", sat, torch.int32, (cameras, height + 1, width + 1))
    want("proj", proj, torch.float32, (cameras, 3, 4))
    want("candidates", candidates, torch.int32, (None,))
    limit = octree_carve_max_cameras()
    if cameras < 1 or cameras > limit:
        raise ValueError("%s: images_u8 holds %d cameras; 1 .. %d are supported (255 * C must be "
                         "exact in f32)" % (who, cameras, limit))
    if not 1 <= height <= 1 << 24 or not 1 <= width <= 1 << 24:
        raise ValueError("%s: images_u8 must be (C, H, W, 4) with 1 <= H, W <= 2^24, got %s"
                         % (who, tuple(images_u8.shape)))
    if height * width >= 2 ** 31:
        raise ValueError("%s: images_u8 has H * W = %d pixels; fewer than 2^31 fit the int32 "
                         "summed-area table" % (who, height * width))
    if not bool(torch.isfinite(proj).all()):
        raise ValueError("%s: proj holds a NaN or an infinity" % who)
    depth, level, expand = int(depth), int(level), bool(expand)
    if depth < 1 or depth > octree_max_depth():
        raise ValueError("%s: depth %d is outside what the path codes hold (1 .. %d)"
                         % (who, depth, octree_max_depth()))
    if not 0 <= level <= depth - 1:
        raise ValueError("%s: level %d is outside 0 .. depth - 1 = %d" % (who, level, depth - 1))
    if expand and level < 1:
        raise ValueError("%s: expand needs level >= 1 (level 0 has no parent)" % who)
    count = candidates.shape[0] * (8 if expand else 1)
    if count < 1 or count > octree_max_points():
        raise ValueError("%s: candidates gives count = %d cells in one call; 1 .. %d fit the scan"
                         % (who, count, octree_max_points()))
    if not 1 <= int(alpha_u8) <= 255:
        raise ValueError("%s: alpha_u8 must lie in 1 .. 255, got %r" % (who, alpha_u8))
    if not 0 <= int(max_misses) < 2 ** 31 or not 0 <= int(min_views) < 2 ** 31:
        raise ValueError("%s: max_misses and min_views must be >= 0, got %r and %r"
                         % (who, max_misses, min_views))
    return cameras, height, width, count


def octree_carve_box_level(images_u8: torch.Tensor, sat: torch.Tensor, proj: torch.Tensor,
                           candidates: torch.Tensor, level: int, center, scale: float, depth: int,
                           alpha_u8: int, max_misses: int, min_views: int, sigma0: float,
                           expand: bool = False, want_visited: bool = False):
    """K27.  One level of the conservative carve.  images_u8 (C,H,W,4) uint8 RGBA, sat (C,H+1,W+1)
    int32 (``octree_carve_box_tables`` of the grown mask), proj (C,3,4) float32, candidates (N,)
    int32: path codes of level ``level`` in code order, or with ``expand`` the codes of N parents of
    level ``level - 1`` whose 8 N children are tested (child ``(parent << 3) | j``), never
    materialised.  -> codes (K) int32 of the survivors in candidate order, and data: (K,4) float32
    ``[r, g, b, sigma0]`` at the finest level (``level == depth - 1``), None below it.  A camera
    refutes a cell only if the padded bounding rectangle of the cell's centre and eight corners lies
    wholly inside the image and holds no foreground pixel; a cell with more than ``max_misses``
    refutations is dropped, and at the finest level also one that fewer than ``min_views`` cameras
    see.  A child's rectangle lies inside its parent's, so the children of a dropped cell need no
    test.  Reads the count back once.  With ``want_visited`` also (count,) int32: how many cameras
    each candidate's loop looked at.  Bad input is a ``ValueError`` (``octree_carve_box_check``)."""
    cameras, height, width, n = octree_carve_box_check(images_u8, sat, proj, candidates, expand,
                                                       level, depth, alpha_u8, max_misses,
                                                       min_views)
    dev = images_u8.device
    rows = torch.empty((n, 4), dtype=torch.float32, device=dev)
    codes = torch.empty((n,), dtype=torch.int32, device=dev)
    data = torch.empty((n, 4), dtype=torch.float32, device=dev)
    total = torch.zeros((), dtype=torch.int32, device=dev)
    visited = torch.empty((n,), dtype=torch.int32, device=dev) if want_visited else None
    flags, offsets, tiles = _scan_scratch(n, dev)
    _call("ffn_octree_carve_box_level", _dev(images_u8, torch.uint8, "images_u8"),
          _dev(sat, torch.int32, "sat"), _dev(proj, name="proj"), c_i(cameras), c_i(height),
          c_i(width), _dev(candidates, torch.int32, "candidates"), c_i64(n),
          c_i(1 if expand else 0), c_i(int(level)), c_f(center[0]), c_f(center[1]),
          c_f(center[2]), c_f(scale), c_i(int(depth)), c_i(int(alpha_u8)), c_i(int(max_misses)),
          c_i(int(min_views)), c_f(sigma0), _dev(flags, torch.uint8), _dev(offsets, torch.int32),
          _dev(tiles, torch.int32), _dev(rows), _dev(visited, torch.int32),
          _dev(codes, torch.int32), _dev(data), _dev(total, torch.int32))
    k = int(total.item())
    kept = data[:k].clone() if int(level) == int(depth) - 1 else None
    if want_visited:
        return codes[:k].clone(), kept, visited
    return codes[:k].clone(), kept


# --------------------------------------------------------------------------------- K24
def octree_visible_check(leaf_centers, leaf_index, rows, stride, sigma_offset, images_u8, proj,
                         eyes, depth, alpha_u8, min_transmittance, out=None, moments=False):
    """The refusals of ``octree_visible_votes`` (and, with ``moments``, of
    ``octree_visible_moments``: its own name, camera limit and eight fields), none of which needs a
    device: shapes, dtypes, contiguity, the camera limit, finite ``proj`` and ``eyes`` (read back
    once), the scalars' ranges.  Tensors on any device.  -> (L, C, H, W).  Raises ``ValueError``
    naming the argument."""
    who = "octree_visible_moments" if moments else "octree_visible_votes"

    def want(name, t, dtype, shape):
        if not torch.is_tensor(t) or t.dtype != dtype:
            raise ValueError("%s: %s must be a %s tensor, got %s"
                             % (who, name, dtype, t.dtype if torch.is_tensor(t) else type(t).__name__))
        if t.dim() != len(shape) or any(w is not None and w != g for w, g in zip(shape, t.shape)):
            raise ValueError("%s: %s must be (%s), got %s"
                             % (who, name, ", ".join("*" if w is None else str(w) for w in shape),
                                tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s: %s must be contiguous" % (who, name))

    want("leaf_index", leaf_index, torch.int64, (None,))
    leaves = leaf_index.shape[0]
    if leaves < 1 or leaves > 1 << 31:
        raise ValueError("%s: leaf_index holds %d leaves; 1 .. 2^31 are supported" % (who, leaves))
    want("leaf_centers", leaf_centers, torch.float32, (leaves, 3))
    stride, sigma_offset = int(stride), int(sigma_offset)
    if stride < 1 or not 0 <= sigma_offset < stride:
        raise ValueError("%s: stride >= 1 and 0 <= sigma_offset < stride, got stride %d, "
                         "sigma_offset %d" % (who, stride, sigma_offset))
    want("rows", rows, torch.float32, (leaves, stride))
    want("images_u8", images_u8, torch.uint8, (None, None, None, 4))
    cameras, height, width = images_u8.shape[:3]
    limit = OCTREE_MOMENTS_MAX_CAMERAS if moments else octree_carve_max_cameras()
    if cameras < 1 or cameras > limit:
        raise ValueError("%s: images_u8 holds %d cameras; 1 .. %d are supported (%s)"
                         % (who, cameras, limit, "255^2 * C must stay below 2^32" if moments
                            else "255 * C must be exact in f32"))
    if not 1 <= height <= 1 << 24 or not 1 <= width <= 1 << 24:
        raise ValueError("%s: images_u8 must be (C, H, W, 4) with 1 <= H, W <= 2^24, got %s"
                         % (who, tuple(images_u8.shape)))
    want("proj", proj, torch.float32, (cameras, 3, 4))
    want("eyes", eyes, torch.float32, (cameras, 3))
    if not bool(torch.isfinite(proj).all()) or not bool(torch.isfinite(eyes).all()):
        raise ValueError("%s: proj or eyes holds a NaN or an infinity" % who)
    depth = int(depth)
    if depth < 1 or depth > octree_max_depth():
        raise ValueError("%s: depth %d is outside what the walk holds (1 .. %d)"
                         % (who, depth, octree_max_depth()))
    if not 1 <= int(alpha_u8) <= 255:
        raise ValueError("%s: alpha_u8 must lie in 1 .. 255, got %r" % (who, alpha_u8))
    _check_min_transmittance("octree visible_moments" if moments else "octree visible_votes",
                             min_transmittance)
    if out is not None:
        want("out", out, torch.uint32, (leaves, 8 if moments else 4))
    return leaves, cameras, height, width


def octree_visible_votes(leaf_centers: torch.Tensor, scale: float, depth: int,
                         node_index: torch.Tensor, leaf_index: torch.Tensor, rows: torch.Tensor,
                         stride: int, sigma_offset: int, images_u8: torch.Tensor,
                         proj: torch.Tensor, eyes: torch.Tensor, alpha_u8: int,
                         min_transmittance: float,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K24.  Per leaf the sum of the pixels of the cameras that see it through the tree as it stands
    -> (L,4) uint32 ``[sum_r, sum_g, sum_b, count]``.  ``leaf_centers`` (L,3) float32 from
    ``octree_leaf_geometry`` (relative to the root cube's centre); ``rows`` / ``stride`` /
    ``sigma_offset`` as for ``octree_leaf_weights`` (only the density is read); ``images_u8``
    (C,H,W,4) uint8 RGBA; ``proj`` (C,3,4) float32 for cube-relative points
    (``cameras.projection_matrices(cameras, origin=center)``) and ``eyes`` (C,3) float32
    (``cameras.eye_positions(cameras, center)``).  Camera c votes for leaf l when the leaf's centre
    projects (K23's operations) onto a pixel of image c whose alpha is ``>= alpha_u8`` and the ray
    from the eye to the centre reaches the leaf before its transmittance, composited as
    ``octree_leaf_weights`` does, falls to ``min_transmittance`` or below.  With ``out`` (L,4)
    uint32 given the votes are ADDED to it (and it is returned): camera subsets folded in several
    calls give the bits of one call, as long as at most ``octree_carve_max_cameras()`` cameras fold
    into one buffer (the caller's count to keep).  Bad input is a ``ValueError``
    (``octree_visible_check``)."""
    return _octree_visible_pairs("ffn_octree_visible_votes", False, leaf_centers, scale, depth,
                                 node_index, leaf_index, rows, stride, sigma_offset, images_u8,
                                 proj, eyes, alpha_u8, min_transmittance, out)


# K28a: 255^2 * C < 2^32 (include/ffn_hip.h); the cameras that may fold into one moments buffer
OCTREE_MOMENTS_MAX_CAMERAS = 66051


def octree_visible_moments(leaf_centers: torch.Tensor, scale: float, depth: int,
                           node_index: torch.Tensor, leaf_index: torch.Tensor, rows: torch.Tensor,
                           stride: int, sigma_offset: int, images_u8: torch.Tensor,
                           proj: torch.Tensor, eyes: torch.Tensor, alpha_u8: int,
                           min_transmittance: float,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K28a.  ``octree_visible_votes`` with the second moments -> (L,8) uint32 ``[sum_r, sum_g,
    sum_b, count, sq_r, sq_g, sq_b, 0]``: the same arguments, the same pairs, and the first four
    fields are the votes bit for bit; ``sq_c`` is the sum of the squares of the seeing cameras'
    bytes.  With ``out`` (L,8) uint32 given the moments are ADDED to it (and it is returned):
    camera subsets folded in several calls, in any order, give the bits of one call, as long as at
    most ``OCTREE_MOMENTS_MAX_CAMERAS`` (66 051: ``255^2 C < 2^32``) cameras fold into one buffer --
    one call takes no more, several are the caller's count to keep.  Bad input is a ``ValueError``
    (``octree_visible_check``)."""
    return _octree_visible_pairs("ffn_octree_visible_moments", True, leaf_centers, scale, depth,
                                 node_index, leaf_index, rows, stride, sigma_offset, images_u8,
                                 proj, eyes, alpha_u8, min_transmittance, out)


def _octree_visible_pairs(entry, moments, leaf_centers, scale, depth, node_index, leaf_index, rows,
                          stride, sigma_offset, images_u8, proj, eyes, alpha_u8, min_transmittance,
                          out):
    """K24 and K28a share their arguments: one check, one call."""
    leaves, cameras, height, width = octree_visible_check(
        leaf_centers, leaf_index, rows, stride, sigma_offset, images_u8, proj, eyes, depth,
        alpha_u8, min_transmittance, out, moments)
    _want("octree_visible_moments" if moments else "octree_visible_votes", "node_index",
          node_index, (None,), torch.int64)
    dev = leaf_index.device
    if out is None:
        out = torch.zeros((leaves, 8 if moments else 4), dtype=torch.uint32, device=dev)
    # per camera 16 floats: P' row-major, the eye, one of padding
    blocks = torch.cat([proj.reshape(cameras, 12), eyes,
                        torch.zeros((cameras, 1), dtype=torch.float32, device=proj.device)],
                       1).contiguous()
    _call(entry, _dev(leaf_centers, name="leaf_centers"), c_i64(leaves),
          c_f(scale), c_i(int(depth)),
          _dev(node_index if node_index.numel() else None, torch.int64, "node_index"),
          c_i64(node_index.numel()), _dev(leaf_index, torch.int64, "leaf_index"),
          _dev(rows, name="rows"), c_i(int(stride)), c_i(int(sigma_offset)),
          _dev(images_u8, torch.uint8, "images_u8"), _dev(blocks, name="camera blocks"),
          c_i(cameras), c_i(height), c_i(width), c_i(int(alpha_u8)), c_f(min_transmittance),
          _dev(out, torch.uint32, "out"))
    return out


# --------------------------------------------------------------------------------- K30
OCTREE_MESH_PLACEMENTS = ("surface_nets", "corners")


def octree_mesh_max_depth() -> int:
    """The deepest tree whose corner keys ``(i (n+1) + j)(n+1) + k`` an int64 holds."""
    fn = _lib.load().ffn_octree_mesh_max_depth
    fn.restype = ctypes.c_int
    return int(fn())


def octree_mesh_check(alpha_threshold, placement):
    """The refusals of K30 that need no device -> (threshold as a float32 value, surface_nets)."""
    if placement not in OCTREE_MESH_PLACEMENTS:
        raise ValueError("octree mesh: placement is 'surface_nets' or 'corners', got %r"
                         % (placement,))
    threshold = float(np.float32(alpha_threshold))
    if not 0.0 < threshold < 1.0:            # NaN fails too
        raise ValueError("octree mesh: alpha_threshold must lie in (0, 1), got %r"
                         % (alpha_threshold,))
    return threshold, placement == "surface_nets"


def octree_mesh_solid(rows: Optional[torch.Tensor], sigma_offset: int,
                      solid: Optional[torch.Tensor], num_leaves: int, side: float,
                      threshold: float, device):
    """K30a.  -> (solid (L,) uint8, alpha (L,) float32): per leaf the opacity over one finest side,
    ``-expm1f(-(sigma * side))`` with ``sigma = rows[:, sigma_offset]`` (0 for a negative or NaN
    sigma), 1 without ``rows``, 1 / 0 from ``solid`` (L,) uint8 when given; solid iff ``alpha >
    threshold``."""
    if rows is not None and (rows.dim() != 2 or rows.shape[0] != num_leaves):
        raise ValueError("octree mesh: rows must be (num_leaves, stride) = (%d, stride), got %s"
                         % (num_leaves, tuple(rows.shape)))
    if rows is not None and not 0 <= int(sigma_offset) < rows.shape[1]:
        raise ValueError("octree mesh: sigma_offset %r is outside the %d columns of rows"
                         % (sigma_offset, rows.shape[1]))
    if solid is not None and tuple(solid.shape) != (num_leaves,):
        raise ValueError("octree mesh: solid must be (num_leaves,) = (%d,), got %s"
                         % (num_leaves, tuple(solid.shape)))
    flags = torch.empty((num_leaves,), dtype=torch.uint8, device=device)
    alpha = torch.empty((num_leaves,), dtype=torch.float32, device=device)
    _call("ffn_octree_mesh_solid", _dev(rows, name="rows"),
          c_i(0 if rows is None else int(rows.shape[1])), c_i(int(sigma_offset)),
          _dev(solid, torch.uint8, "solid"), c_i64(num_leaves), c_f(side), c_f(threshold),
          _dev(flags, torch.uint8, "flags"), _dev(alpha, name="alpha"))
    return flags, alpha


def octree_mesh_candidate_offsets(leaf_index: torch.Tensor, solid: torch.Tensor, depth: int):
    """The exclusive int64 scan behind K30b -> (offsets (L+1,) int64 on the device, total, deepest
    level; one read-back).  A solid leaf of ``k = 2^(depth-1-level)`` cells a side has ``6 k^2 + 2``
    corners on its closed surface; a leaf that is not solid has none.  Integer plumbing."""
    dev = leaf_index.device
    limit = octree_mesh_max_depth()
    first_id = torch.tensor([(8 ** k - 1) // 7 for k in range(limit + 1)], dtype=torch.int64,
                            device=dev)
    levels = torch.searchsorted(first_id, leaf_index, right=True) - 1
    cells = torch.ones_like(levels) << (depth - 1 - levels).clamp(min=0)
    counts = torch.where(solid != 0, 6 * cells * cells + 2, torch.zeros_like(cells))
    offsets = torch.zeros((leaf_index.numel() + 1,), dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=offsets[1:])
    total, top_level = torch.stack([offsets[-1], levels.max()]).cpu().tolist()
    return offsets, int(total), int(top_level)


def octree_mesh_candidates(node_index: torch.Tensor, leaf_index: torch.Tensor,
                           solid: torch.Tensor, cand_offsets: torch.Tensor, first: int,
                           count: int, depth: int):
    """K30b on the candidates ``first .. first + count - 1`` -> (keys (K,) int64, masks (K,) uint8,
    samples (K,8) int32) of the corners kept, in candidate order.  Reads the count back once."""
    _want_tensors("octree mesh", leaf_index=leaf_index, solid=solid, cand_offsets=cand_offsets)
    _want("octree mesh", "node_index", node_index, (None,), torch.int64)
    _want_int("octree mesh", "depth", depth, 1, octree_mesh_max_depth())
    dev = leaf_index.device
    num_leaves = leaf_index.numel()
    if tuple(solid.shape) != (num_leaves,) or tuple(cand_offsets.shape) != (num_leaves + 1,):
        raise ValueError("octree mesh: solid (num_leaves,) and cand_offsets (num_leaves + 1,) must "
                         "fit the %d leaves, got %s and %s"
                         % (num_leaves, tuple(solid.shape), tuple(cand_offsets.shape)))
    if count < 1 or count > octree_max_points():
        raise ValueError("octree mesh: 1 <= count <= %d candidates a call, got %d"
                         % (octree_max_points(), count))
    flags, offsets, tiles = _scan_scratch(count, dev)
    keys = torch.empty((2, count), dtype=torch.int64, device=dev)
    masks = torch.empty((2, count), dtype=torch.uint8, device=dev)
    samples = torch.empty((2, count, 8), dtype=torch.int32, device=dev)
    total = torch.zeros((), dtype=torch.int32, device=dev)
    _call("ffn_octree_mesh_candidates",
          _dev(node_index if node_index.numel() else None, torch.int64, "node_index"),
          c_i64(node_index.numel()), _dev(leaf_index, torch.int64, "leaf_index"),
          c_i64(num_leaves), _dev(solid, torch.uint8, "solid"),
          _dev(cand_offsets, torch.int64, "cand_offsets"), c_i64(first), c_i64(count),
          c_i(int(depth)), _dev(flags, torch.uint8), _dev(offsets, torch.int32),
          _dev(tiles, torch.int32), _dev(keys[0], torch.int64), _dev(masks[0], torch.uint8),
          _dev(samples[0], torch.int32), _dev(keys[1], torch.int64), _dev(masks[1], torch.uint8),
          _dev(samples[1], torch.int32), _dev(total, torch.int32))
    k = int(total.item())
    return keys[1, :k].clone(), masks[1, :k].clone(), samples[1, :k].clone()


def octree_mesh_vertices(keys: torch.Tensor, masks: torch.Tensor, samples: torch.Tensor,
                         alpha: torch.Tensor, rows: Optional[torch.Tensor], color, depth: int,
                         scale: float, center, threshold: float, surface_nets: bool):
    """K30c.  ``keys`` (V,) int64 ascending with their ``masks`` (V,) uint8 and ``samples`` (V,8)
    int32; ``alpha`` (L,) of K30a; ``rows`` (L, stride) and ``color = (offset, step, sh)`` name the
    three colour columns (``sh``: band-0 SH logits), or ``rows`` None for no colours.
    -> vertices (V,3) f32, colors (V,3) f32 or None, normals (V,3) f32, corners (V,3) int32."""
    _want("octree mesh", "keys", keys, (None,), torch.int64)
    _want_tensors("octree mesh", masks=masks, samples=samples)
    _want("octree mesh", "alpha", alpha, (None,))
    dev = keys.device
    count = keys.numel()
    num_leaves = alpha.numel()
    if tuple(masks.shape) != (count,) or tuple(samples.shape) != (count, 8):
        raise ValueError("octree mesh: keys (V,), masks (V,) and samples (V,8) disagree: %s, %s, %s"
                         % (tuple(keys.shape), tuple(masks.shape), tuple(samples.shape)))
    if rows is not None and (rows.dim() != 2 or rows.shape[0] != num_leaves):
        raise ValueError("octree mesh: rows must be (num_leaves, stride) = (%d, stride), got %s"
                         % (num_leaves, tuple(rows.shape)))
    vertices = torch.empty((count, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((count, 3), dtype=torch.float32, device=dev)
    corners = torch.empty((count, 3), dtype=torch.int32, device=dev)
    colors = None if rows is None else torch.empty((count, 3), dtype=torch.float32, device=dev)
    if count == 0:
        return vertices, colors, normals, corners
    offset, step, sh = (0, 1, 0) if rows is None else [int(v) for v in color]
    _call("ffn_octree_mesh_vertices", _dev(keys, torch.int64, "keys"),
          _dev(masks, torch.uint8, "masks"), _dev(samples, torch.int32, "samples"), c_i64(count),
          _dev(alpha, name="alpha"), _dev(rows, name="rows"), c_i64(num_leaves),
          c_i(0 if rows is None else int(rows.shape[1])), c_i(offset), c_i(step), c_i(sh),
          c_i(int(depth)), c_f(scale), c_f(center[0]), c_f(center[1]), c_f(center[2]),
          c_f(threshold), c_i(int(bool(surface_nets))), _dev(vertices), _dev(colors),
          _dev(normals), _dev(corners, torch.int32))
    return vertices, colors, normals, corners


def octree_mesh_faces(keys: torch.Tensor, masks: torch.Tensor, depth: int) -> torch.Tensor:
    """K30d.  ``keys`` (V,) int64 ascending and their ``masks`` -> triangles (F,3) int32, two per
    owned quad, ordered by owner vertex, then axis, wound so that the normal points from solid to
    empty.  Reads the quad count back once; a quad whose corner is not among the keys raises."""
    _want("octree mesh", "keys", keys, (None,), torch.int64)
    _want_tensors("octree mesh", masks=masks)
    dev = keys.device
    count = keys.numel()
    if tuple(masks.shape) != (count,):
        raise ValueError("octree mesh: keys (V,) and masks (V,) disagree: %s, %s"
                         % (tuple(keys.shape), tuple(masks.shape)))
    if count == 0:
        return torch.empty((0, 3), dtype=torch.int32, device=dev)
    if 3 * count > octree_max_points():
        raise ValueError("octree mesh: %d vertices are more than one face scan holds (%d)"
                         % (count, octree_max_points() // 3))
    flags, offsets, tiles = _scan_scratch(3 * count, dev)
    total = torch.zeros((), dtype=torch.int32, device=dev)
    _call("ffn_octree_mesh_face_flags", _dev(masks, torch.uint8, "masks"), c_i64(count),
          _dev(flags, torch.uint8), _dev(offsets, torch.int32), _dev(tiles, torch.int32),
          _dev(total, torch.int32))
    quads = int(total.item())
    triangles = torch.empty((2 * quads, 3), dtype=torch.int32, device=dev)
    if quads == 0:
        return triangles
    missing = torch.zeros((1,), dtype=torch.int32, device=dev)
    _call("ffn_octree_mesh_faces", _dev(keys, torch.int64, "keys"),
          _dev(masks, torch.uint8, "masks"), _dev(flags, torch.uint8), _dev(offsets, torch.int32),
          c_i64(count), c_i(int(depth)), c_i64(quads), _dev(triangles, torch.int32),
          _dev(missing, torch.int32))
    return triangles


# --------------------------------------------------------------------------------- K31
MESH_RASTER_MAX_SIDE = 16384
MESH_RASTER_STATUS = ("drawn", "behind", "clipped", "degenerate", "off_image")
MESH_RASTER_EMPTY = -1              # a z-buffer entry of all ones, as the int64 torch holds


def _raster_want(who, name, t, dtype, shape):
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise ValueError("%s: %s must be a %s tensor, got %s"
                         % (who, name, dtype, t.dtype if torch.is_tensor(t) else type(t).__name__))
    if t.dim() != len(shape) or any(w is not None and w != g for w, g in zip(shape, t.shape)):
        raise ValueError("%s: %s must be (%s), got %s"
                         % (who, name, ", ".join("*" if w is None else str(w) for w in shape),
                            tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous" % (who, name))


def _raster_check_image(who, width, height):
    if not 1 <= width <= MESH_RASTER_MAX_SIDE or not 1 <= height <= MESH_RASTER_MAX_SIDE:
        raise ValueError("%s: width and height must lie in 1 .. %d, got %d x %d"
                         % (who, MESH_RASTER_MAX_SIDE, width, height))


def _raster_check_mesh(who, vertices, triangles):
    _raster_want(who, "vertices", vertices, torch.float32, (None, 3))
    _raster_want(who, "triangles", triangles, torch.int32, (None, 3))
    most = (2 ** 31 - 1) // 3
    if not 1 <= vertices.shape[0] <= most:
        raise ValueError("%s: vertices holds %d vertices; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, vertices.shape[0]))
    if not 1 <= triangles.shape[0] <= most:
        raise ValueError("%s: triangles holds %d triangles; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, triangles.shape[0]))


def _raster_host(who, name, values, count):
    arr = np.asarray(values, dtype=np.float32).reshape(-1)
    if arr.shape != (count,) or not np.isfinite(arr).all():
        raise ValueError("%s: %s must be %d finite numbers, got %r" % (who, name, count, values))
    return (ctypes.c_float * count)(*arr.tolist())


def mesh_raster_setup_check(vertices, triangles, proj, width: int, height: int):
    """The refusals of ``mesh_raster_setup``, none of which needs a device -> ``proj`` as 12 host
    floats.  Raises ``ValueError`` naming the argument."""
    who = "mesh_raster_setup"
    _raster_check_mesh(who, vertices, triangles)
    _raster_check_image(who, width, height)
    if np.shape(proj) != (3, 4):
        raise ValueError("%s: proj must be (3, 4), got %s" % (who, np.shape(proj)))
    return _raster_host(who, "proj", proj, 12)


def mesh_raster_setup(vertices: torch.Tensor, triangles: torch.Tensor, proj, width: int,
                      height: int):
    """K31a.  vertices (V,3) f32, triangles (F,3) int32, ``proj`` (3,4) on the host (one matrix of
    ``cameras.projection_matrices``) -> ``(record (F,16) int32, status (F,) uint8, counts (F,)
    int64)``: the snapped vertices, ``w`` and pixel box of every triangle, its status (an index
    into ``MESH_RASTER_STATUS``) and its number of box pixels, 0 unless it is drawn.  There is no
    near-plane clipping: a triangle that crosses ``w = 0`` or leaves the guard band of 16384
    pixels has the status ``clipped`` and is not drawn."""
    width, height = int(width), int(height)
    matrix = mesh_raster_setup_check(vertices, triangles, proj, width, height)
    dev = vertices.device
    num = triangles.shape[0]
    record = torch.empty((num, 16), dtype=torch.int32, device=dev)
    status = torch.empty((num,), dtype=torch.uint8, device=dev)
    counts = torch.empty((num,), dtype=torch.int64, device=dev)
    _call("ffn_mesh_raster_setup", _dev(vertices, name="vertices"), c_i64(vertices.shape[0]),
          _dev(triangles, torch.int32, "triangles"), c_i64(num), matrix, c_i(width), c_i(height),
          _dev(record, torch.int32), _dev(status, torch.uint8), _dev(counts, torch.int64))
    return record, status, counts


def mesh_raster_offsets(counts: torch.Tensor):
    """The exclusive int64 scan behind K31b -> (offsets (F+1,) int64 on the device, total; one
    read-back).  Integer plumbing, as ``octree_mesh_candidate_offsets``."""
    offsets = torch.zeros((counts.numel() + 1,), dtype=torch.int64, device=counts.device)
    torch.cumsum(counts, 0, out=offsets[1:])
    return offsets, int(offsets[-1].item())


def mesh_raster_draw_check(record, offsets, first: int, count: int, width: int, height: int,
                           zbuf) -> None:
    """The refusals of ``mesh_raster_draw`` that need no device."""
    who = "mesh_raster_draw"
    _raster_want(who, "record", record, torch.int32, (None, 16))
    _raster_want(who, "offsets", offsets, torch.int64, (record.shape[0] + 1,))
    _raster_check_image(who, width, height)
    _raster_want(who, "zbuf", zbuf, torch.int64, (width * height,))
    if record.shape[0] < 1:
        raise ValueError("%s: record holds no triangle" % who)
    if first < 0 or not 1 <= count <= octree_max_points():
        raise ValueError("%s: first >= 0 and 1 <= count <= %d, got first %d, count %d"
                         % (who, octree_max_points(), first, count))


def mesh_raster_draw(record: torch.Tensor, offsets: torch.Tensor, first: int, count: int,
                     width: int, height: int, zbuf: torch.Tensor) -> torch.Tensor:
    """K31b on the box pixels ``first .. first + count - 1`` of the scan ``offsets``: every covered
    one lowers ``zbuf`` (H W,) int64, ``MESH_RASTER_EMPTY`` where nothing was drawn, to
    ``bits(depth_w) << 32 | triangle`` when that is less (as unsigned).  The caller keeps
    ``first + count`` within the scan's total.  -> ``zbuf``."""
    first, count, width, height = int(first), int(count), int(width), int(height)
    mesh_raster_draw_check(record, offsets, first, count, width, height, zbuf)
    _call("ffn_mesh_raster_draw", _dev(record, torch.int32, "record"),
          _dev(offsets, torch.int64, "offsets"), c_i64(record.shape[0]), c_i64(first),
          c_i64(count), c_i(width), c_i(height), _dev(zbuf, torch.int64, "zbuf"))
    return zbuf


def mesh_raster_resolve_check(zbuf, record, vertices, triangles, colors, uvs, texture, eye,
                              background, width: int, height: int):
    """The refusals of ``mesh_raster_resolve`` that need no device -> (eye, background) as host
    floats.  Exactly one of ``colors`` and ``uvs`` + ``texture`` is given."""
    who = "mesh_raster_resolve"
    _raster_check_mesh(who, vertices, triangles)
    _raster_check_image(who, width, height)
    _raster_want(who, "record", record, torch.int32, (triangles.shape[0], 16))
    _raster_want(who, "zbuf", zbuf, torch.int64, (width * height,))
    if (colors is None) == (uvs is None and texture is None) or (uvs is None) != (texture is None):
        raise ValueError("%s: give either colors, or uvs and texture" % who)
    if colors is not None:
        _raster_want(who, "colors", colors, torch.float32, (vertices.shape[0], 3))
    else:
        _raster_want(who, "uvs", uvs, torch.float32, (vertices.shape[0], 2))
        _raster_want(who, "texture", texture, torch.uint8, (None, None, None))
        tex_h, tex_w, channels = texture.shape
        if (channels < 3 or not 1 <= tex_h <= MESH_MAX_TEXTURE_SIDE
                or not 1 <= tex_w <= MESH_MAX_TEXTURE_SIDE or tex_h * tex_w * channels >= 2 ** 31):
            raise ValueError("%s: texture must be (H, W, C) with C >= 3, 1 <= H, W <= 2^24 and "
                             "fewer than 2^31 bytes, got %s" % (who, tuple(texture.shape)))
    return _raster_host(who, "eye", eye, 3), _raster_host(who, "background", background, 3)


def mesh_raster_resolve(zbuf: torch.Tensor, record: torch.Tensor, vertices: torch.Tensor,
                        triangles: torch.Tensor, colors: Optional[torch.Tensor],
                        uvs: Optional[torch.Tensor], texture: Optional[torch.Tensor], eye,
                        background, width: int, height: int):
    """K31c.  -> ``(color (H W,3), alpha (H W,), depth (H W,) float32, ids (H W,) int32)``: per
    pixel the winning triangle's perspective-correct colour (``colors`` (V,3), or ``uvs`` (V,2)
    through ``texture`` (h,w,C) uint8 with the row index growing with ``v``, K22's lookup), 1, the
    distance of the surface point from ``eye`` and the triangle's number; ``background``, 0, 0 and
    -1 where nothing was drawn."""
    width, height = int(width), int(height)
    eye_c, background_c = mesh_raster_resolve_check(zbuf, record, vertices, triangles, colors, uvs,
                                                    texture, eye, background, width, height)
    dev = vertices.device
    n = width * height
    color = torch.empty((n, 3), dtype=torch.float32, device=dev)
    alpha = torch.empty((n,), dtype=torch.float32, device=dev)
    depth = torch.empty((n,), dtype=torch.float32, device=dev)
    ids = torch.empty((n,), dtype=torch.int32, device=dev)
    tex_h, tex_w, channels = (0, 0, 0) if texture is None else texture.shape
    _call("ffn_mesh_raster_resolve", _dev(zbuf, torch.int64, "zbuf"),
          _dev(record, torch.int32, "record"), _dev(vertices, name="vertices"),
          c_i64(vertices.shape[0]), _dev(triangles, torch.int32, "triangles"),
          c_i64(triangles.shape[0]), _dev(colors, name="colors"), _dev(uvs, name="uvs"),
          _dev(texture, torch.uint8, "texture"), c_i(tex_h), c_i(tex_w), c_i(channels), eye_c,
          background_c, c_i(width), c_i(height), _dev(color), _dev(alpha), _dev(depth),
          _dev(ids, torch.int32))
    return color, alpha, depth, ids


# --------------------------------------------------------------------------------- K32
def mesh_raster_face_sums_check(record, ids, d_color, width: int, height: int) -> None:
    """The refusals of ``mesh_raster_face_sums`` that need no device."""
    who = "mesh_raster_face_sums"
    _raster_want(who, "record", record, torch.int32, (None, 16))
    _raster_check_image(who, width, height)
    _raster_want(who, "ids", ids, torch.int32, (width * height,))
    _raster_want(who, "d_color", d_color, torch.float32, (width * height, 3))
    if not 1 <= record.shape[0] <= (2 ** 31 - 1) // 3:
        raise ValueError("%s: record holds %d triangles; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, record.shape[0]))


def mesh_raster_face_sums(record: torch.Tensor, ids: torch.Tensor, d_color: torch.Tensor,
                          width: int, height: int) -> torch.Tensor:
    """K32a.  record (F,16) int32 of K31a, ids (H W,) int32 of K31c, d_color (H W,3) f32 ->
    ``face_sums`` (F,12) f32: per triangle, over the pixels ``ids`` gives it, the sums of
    ``b_i * d_color[p][j]`` (columns ``3 i + j``) and of ``b_i`` (columns ``9 + i``), ``b_i`` the
    barycentric weights of K31c; one wavefront per triangle, a fixed order, no atomics.  A pixel
    whose id is another triangle's (or -1) is not read: a NaN there reaches nothing."""
    width, height = int(width), int(height)
    mesh_raster_face_sums_check(record, ids, d_color, width, height)
    face_sums = torch.empty((record.shape[0], 12), dtype=torch.float32, device=record.device)
    _call("ffn_mesh_raster_face_sums", _dev(record, torch.int32, "record"),
          _dev(ids, torch.int32, "ids"), _dev(d_color, name="d_color"), c_i64(record.shape[0]),
          c_i(width), c_i(height), _dev(face_sums))
    return face_sums


def mesh_vertex_gather_check(face_sums, corner_order, vertex_starts, grad=None, weight=None,
                             accumulate: bool = False) -> int:
    """The refusals of ``mesh_vertex_gather`` that need no device -> the number of vertices."""
    who = "mesh_vertex_gather"
    _raster_want(who, "face_sums", face_sums, torch.float32, (None, 12))
    most = (2 ** 31 - 1) // 3
    if not 1 <= face_sums.shape[0] <= most:
        raise ValueError("%s: face_sums holds %d triangles; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, face_sums.shape[0]))
    _raster_want(who, "corner_order", corner_order, torch.int32, (3 * face_sums.shape[0],))
    _raster_want(who, "vertex_starts", vertex_starts, torch.int32, (None,))
    num_vertices = vertex_starts.shape[0] - 1
    if not 1 <= num_vertices <= most:
        raise ValueError("%s: vertex_starts must be (V + 1,) with 1 <= V <= (2^31 - 1) / 3, got "
                         "%s" % (who, tuple(vertex_starts.shape)))
    if (grad is None) != (weight is None):
        raise ValueError("%s: give both grad and weight, or neither" % who)
    if accumulate and grad is None:
        raise ValueError("%s: accumulate needs grad and weight to add to" % who)
    if grad is not None:
        _raster_want(who, "grad", grad, torch.float32, (num_vertices, 3))
        _raster_want(who, "weight", weight, torch.float32, (num_vertices,))
    return num_vertices


def mesh_vertex_gather(face_sums: torch.Tensor, corner_order: torch.Tensor,
                       vertex_starts: torch.Tensor, grad: Optional[torch.Tensor] = None,
                       weight: Optional[torch.Tensor] = None, accumulate: bool = False):
    """K32b.  face_sums (F,12) of K32a, ``corner_order`` (3F,) int32 and ``vertex_starts`` (V+1,)
    int32 of ``mesh.vertex_adjacency`` -> ``(grad (V,3), weight (V,))`` f32: per vertex the sums of
    its corners' rows of ``face_sums`` in CSR order, one thread per vertex.  ``grad`` and ``weight``
    are written in place when given, and with ``accumulate`` added to (``out = out + value``)."""
    num_vertices = mesh_vertex_gather_check(face_sums, corner_order, vertex_starts, grad, weight,
                                            accumulate)
    if grad is None:
        grad = torch.empty((num_vertices, 3), dtype=torch.float32, device=face_sums.device)
        weight = torch.empty((num_vertices,), dtype=torch.float32, device=face_sums.device)
    _call("ffn_mesh_vertex_gather", _dev(face_sums, name="face_sums"),
          _dev(corner_order, torch.int32, "corner_order"),
          _dev(vertex_starts, torch.int32, "vertex_starts"), c_i64(face_sums.shape[0]),
          c_i64(num_vertices), _dev(grad, name="grad"), _dev(weight, name="weight"),
          c_i(1 if accumulate else 0))
    return grad, weight


# --------------------------------------------------------------------------------- K33
MESH_TEXTURE_MAX_TEXELS = (2 ** 31 - 1) // 3    # 3 T floats index in an int32
MESH_TEXTURE_MAX_PIXELS = 1 << 28               # 4 P tap slots index in an int32


def _texture_check_size(who, tex_height, tex_width):
    if (not 1 <= tex_height <= MESH_MAX_TEXTURE_SIDE or not 1 <= tex_width <= MESH_MAX_TEXTURE_SIDE
            or tex_height * tex_width > MESH_TEXTURE_MAX_TEXELS):
        raise ValueError("%s: the texture must be 1 .. 2^24 a side with at most (2^31 - 1) / 3 "
                         "texels, got %d x %d" % (who, tex_height, tex_width))


def _texture_check_taps(who, tap_texel, tap_weight) -> int:
    _raster_want(who, "tap_texel", tap_texel, torch.int32, (None, 4))
    num_pixels = tap_texel.shape[0]
    if not 1 <= num_pixels <= MESH_TEXTURE_MAX_PIXELS:
        raise ValueError("%s: tap_texel holds %d pixels; 1 .. 2^28 are supported"
                         % (who, num_pixels))
    _raster_want(who, "tap_weight", tap_weight, torch.float32, (num_pixels, 4))
    return num_pixels


def mesh_texture_taps_check(record, ids, triangles, uvs, tex_height: int, tex_width: int,
                            width: int, height: int) -> None:
    """The refusals of ``mesh_texture_taps`` that need no device."""
    who = "mesh_texture_taps"
    _raster_want(who, "triangles", triangles, torch.int32, (None, 3))
    _raster_want(who, "uvs", uvs, torch.float32, (None, 2))
    most = (2 ** 31 - 1) // 3
    if not 1 <= triangles.shape[0] <= most:
        raise ValueError("%s: triangles holds %d triangles; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, triangles.shape[0]))
    if not 1 <= uvs.shape[0] <= most:
        raise ValueError("%s: uvs holds %d vertices; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, uvs.shape[0]))
    _raster_want(who, "record", record, torch.int32, (triangles.shape[0], 16))
    _raster_check_image(who, width, height)
    _raster_want(who, "ids", ids, torch.int32, (width * height,))
    _texture_check_size(who, tex_height, tex_width)


def mesh_texture_taps(record: torch.Tensor, ids: torch.Tensor, triangles: torch.Tensor,
                      uvs: torch.Tensor, tex_height: int, tex_width: int, width: int, height: int):
    """K33a.  record (F,16) int32 of K31a, ids (H W,) int32 of K31c, triangles (F,3) int32, uvs
    (V,2) f32 and the size of the texture -> ``(tap_texel (H W,4) int32, tap_weight (H W,4) f32)``:
    per pixel the four texels ``i * tex_width + j`` K31c's bilinear lookup blends, in the order 00,
    01, 10, 11, and their weights, the bits K31c uses.  A pixel whose id is outside ``0 .. F - 1``
    is uncovered: texels -1, weights +0."""
    tex_height, tex_width = int(tex_height), int(tex_width)
    width, height = int(width), int(height)
    mesh_texture_taps_check(record, ids, triangles, uvs, tex_height, tex_width, width, height)
    tap_texel = torch.empty((width * height, 4), dtype=torch.int32, device=record.device)
    tap_weight = torch.empty((width * height, 4), dtype=torch.float32, device=record.device)
    _call("ffn_mesh_texture_taps", _dev(record, torch.int32, "record"),
          _dev(ids, torch.int32, "ids"), _dev(triangles, torch.int32, "triangles"),
          c_i64(triangles.shape[0]), _dev(uvs, name="uvs"), c_i64(uvs.shape[0]), c_i(tex_height),
          c_i(tex_width), c_i(width), c_i(height), _dev(tap_texel, torch.int32),
          _dev(tap_weight))
    return tap_texel, tap_weight


def mesh_texture_gather_check(tap_texel, tap_weight, texture, background):
    """The refusals of ``mesh_texture_gather`` that need no device -> ``background`` as 3 host
    floats."""
    who = "mesh_texture_gather"
    _texture_check_taps(who, tap_texel, tap_weight)
    _raster_want(who, "texture", texture, torch.float32, (None, 3))
    if not 1 <= texture.shape[0] <= MESH_TEXTURE_MAX_TEXELS:
        raise ValueError("%s: texture holds %d texels; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, texture.shape[0]))
    return _raster_host(who, "background", background, 3)


def mesh_texture_gather(tap_texel: torch.Tensor, tap_weight: torch.Tensor, texture: torch.Tensor,
                        background=(0, 0, 0)):
    """K33b.  The taps of K33a and ``texture`` (T,3) f32, plain floats -> ``(color (P,3), alpha
    (P,))`` f32: ``((w00 t00 + w01 t01) + w10 t10) + w11 t11`` per channel and 1 for a covered
    pixel, ``background`` and 0 for an uncovered one (``tap_texel[p][0] < 0``).  A tap whose texel
    is outside ``0 .. T - 1`` contributes +0."""
    background_c = mesh_texture_gather_check(tap_texel, tap_weight, texture, background)
    num_pixels = tap_texel.shape[0]
    color = torch.empty((num_pixels, 3), dtype=torch.float32, device=tap_texel.device)
    alpha = torch.empty((num_pixels,), dtype=torch.float32, device=tap_texel.device)
    _call("ffn_mesh_texture_gather", _dev(tap_texel, torch.int32, "tap_texel"),
          _dev(tap_weight, name="tap_weight"), _dev(texture, name="texture"),
          c_i64(texture.shape[0]), background_c, c_i64(num_pixels), _dev(color), _dev(alpha))
    return color, alpha


def mesh_texture_grad_check(sorted_texels, tap_order, tap_weight, d_color, num_texels: int,
                            grad=None, weight=None, accumulate: bool = False) -> int:
    """The refusals of ``mesh_texture_grad`` that need no device -> the number of pixels."""
    who = "mesh_texture_grad"
    _raster_want(who, "tap_weight", tap_weight, torch.float32, (None, 4))
    num_pixels = tap_weight.shape[0]
    if not 1 <= num_pixels <= MESH_TEXTURE_MAX_PIXELS:
        raise ValueError("%s: tap_weight holds %d pixels; 1 .. 2^28 are supported"
                         % (who, num_pixels))
    _raster_want(who, "sorted_texels", sorted_texels, torch.int32, (4 * num_pixels,))
    _raster_want(who, "tap_order", tap_order, torch.int32, (4 * num_pixels,))
    _raster_want(who, "d_color", d_color, torch.float32, (num_pixels, 3))
    if int(num_texels) != num_texels or not 1 <= num_texels <= MESH_TEXTURE_MAX_TEXELS:
        raise ValueError("%s: num_texels must be an integer in 1 .. (2^31 - 1) / 3, got %r"
                         % (who, num_texels))
    if (grad is None) != (weight is None):
        raise ValueError("%s: give both grad and weight, or neither" % who)
    if accumulate and grad is None:
        raise ValueError("%s: accumulate needs grad and weight to add to" % who)
    if grad is not None:
        _raster_want(who, "grad", grad, torch.float32, (int(num_texels), 3))
        _raster_want(who, "weight", weight, torch.float32, (int(num_texels),))
    return num_pixels


def mesh_texture_grad(sorted_texels: torch.Tensor, tap_order: torch.Tensor,
                      tap_weight: torch.Tensor, d_color: torch.Tensor, num_texels: int,
                      grad: Optional[torch.Tensor] = None, weight: Optional[torch.Tensor] = None,
                      accumulate: bool = False):
    """K33c.  ``sorted_texels`` and ``tap_order`` (4P,) int32: the tap slots ``4 p + k`` stably
    sorted by ``tap_texel`` (``mesh.mesh_texture_taps`` makes them); ``tap_weight`` (P,4) and
    ``d_color`` (P,3) f32 -> ``(grad (T,3), weight (T,))`` f32: per texel, over its taps in sorted
    order, the sums of ``w * d_color[p]`` and of ``w``; a tap with ``!(w > 0)`` is skipped, so a NaN
    weight reaches no texel.  One thread per texel, no atomics.  ``grad`` and ``weight`` are written
    in place when given, and with ``accumulate`` added to (``out = out + value``)."""
    num_pixels = mesh_texture_grad_check(sorted_texels, tap_order, tap_weight, d_color,
                                         num_texels, grad, weight, accumulate)
    num_texels = int(num_texels)
    if grad is None:
        grad = torch.empty((num_texels, 3), dtype=torch.float32, device=tap_weight.device)
        weight = torch.empty((num_texels,), dtype=torch.float32, device=tap_weight.device)
    _call("ffn_mesh_texture_grad", _dev(sorted_texels, torch.int32, "sorted_texels"),
          _dev(tap_order, torch.int32, "tap_order"), _dev(tap_weight, name="tap_weight"),
          _dev(d_color, name="d_color"), c_i64(num_pixels), c_i64(num_texels),
          _dev(grad, name="grad"), _dev(weight, name="weight"), c_i(1 if accumulate else 0))
    return grad, weight


# --------------------------------------------------------------------------------- K34
MESH_AA_MAX_PIXELS = 1 << 28                    # 4 P entries index in an int32


def _aa_check_frame(who, record, zbuf, ids, opposite, vertices, proj, color, alpha, width, height):
    """What K34a and K34b refuse alike -> ``proj`` as 12 host floats."""
    _raster_want(who, "vertices", vertices, torch.float32, (None, 3))
    _raster_want(who, "record", record, torch.int32, (None, 16))
    most = (2 ** 31 - 1) // 3
    if not 1 <= vertices.shape[0] <= most:
        raise ValueError("%s: vertices holds %d vertices; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, vertices.shape[0]))
    if not 1 <= record.shape[0] <= most:
        raise ValueError("%s: record holds %d triangles; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, record.shape[0]))
    _raster_check_image(who, width, height)
    if width * height > MESH_AA_MAX_PIXELS:
        raise ValueError("%s: the image holds %d pixels; at most 2^28 are supported"
                         % (who, width * height))
    _raster_want(who, "zbuf", zbuf, torch.int64, (width * height,))
    _raster_want(who, "ids", ids, torch.int32, (width * height,))
    _raster_want(who, "opposite", opposite, torch.int32, (3 * record.shape[0],))
    _raster_want(who, "color", color, torch.float32, (width * height, 3))
    _raster_want(who, "alpha", alpha, torch.float32, (width * height,))
    if np.shape(proj) != (3, 4):
        raise ValueError("%s: proj must be (3, 4), got %s" % (who, np.shape(proj)))
    return _raster_host(who, "proj", proj, 12)


def mesh_aa_forward_check(record, zbuf, ids, opposite, vertices, proj, color, alpha, width: int,
                          height: int):
    """The refusals of ``mesh_aa_forward`` that need no device -> ``proj`` as 12 host floats."""
    return _aa_check_frame("mesh_aa_forward", record, zbuf, ids, opposite, vertices, proj, color,
                           alpha, width, height)


def mesh_aa_forward(record: torch.Tensor, zbuf: torch.Tensor, ids: torch.Tensor,
                    opposite: torch.Tensor, vertices: torch.Tensor, proj, color: torch.Tensor,
                    alpha: torch.Tensor, width: int, height: int):
    """K34a.  record (F,16) of K31a, zbuf (H W,) int64 of K31b, ids, color (H W,3) and alpha (H W,)
    of K31c, ``opposite`` (3F,) int32 of ``mesh.edge_opposites``, vertices (V,3) f32 and ``proj``
    (3,4) on the host -> ``(out_color (H W,3), out_alpha (H W,))`` f32: every pair of 4-neighbours
    with different ids that a silhouette edge separates is blended by how far the edge reaches
    between the two centres, ``out = out + m * (in[source] - in[p])`` at the pair's target.  A pixel
    in no such pair is copied bit for bit."""
    width, height = int(width), int(height)
    matrix = mesh_aa_forward_check(record, zbuf, ids, opposite, vertices, proj, color, alpha,
                                   width, height)
    out_color, out_alpha = torch.empty_like(color), torch.empty_like(alpha)
    _call("ffn_mesh_aa_forward", _dev(record, torch.int32, "record"),
          _dev(zbuf, torch.int64, "zbuf"), _dev(ids, torch.int32, "ids"),
          _dev(opposite, torch.int32, "opposite"), _dev(vertices, name="vertices"),
          c_i64(vertices.shape[0]), c_i64(record.shape[0]), matrix, _dev(color, name="color"),
          _dev(alpha, name="alpha"), c_i(width), c_i(height), _dev(out_color), _dev(out_alpha))
    return out_color, out_alpha


def mesh_aa_backward_check(record, zbuf, ids, opposite, vertices, triangles, proj, color, alpha,
                           g_color, g_alpha, width: int, height: int):
    """The refusals of ``mesh_aa_backward`` that need no device -> ``proj`` as 12 host floats."""
    who = "mesh_aa_backward"
    matrix = _aa_check_frame(who, record, zbuf, ids, opposite, vertices, proj, color, alpha, width,
                             height)
    _raster_want(who, "triangles", triangles, torch.int32, (record.shape[0], 3))
    _raster_want(who, "g_color", g_color, torch.float32, (width * height, 3))
    _raster_want(who, "g_alpha", g_alpha, torch.float32, (width * height,))
    return matrix


def mesh_aa_backward(record: torch.Tensor, zbuf: torch.Tensor, ids: torch.Tensor,
                     opposite: torch.Tensor, vertices: torch.Tensor, triangles: torch.Tensor, proj,
                     color: torch.Tensor, alpha: torch.Tensor, g_color: torch.Tensor,
                     g_alpha: torch.Tensor, width: int, height: int):
    """K34b.  The inputs of ``mesh_aa_forward``, ``triangles`` (F,3) int32 and the gradient
    ``g_color`` (H W,3), ``g_alpha`` (H W,) in its outputs -> ``(d_color (H W,3), d_alpha (H W,),
    entry_vertex (4 H W,) int32, entry_grad (4 H W,2) f32)``: the gradient in K31c's colour and
    alpha (the transpose of the blend), and per slot ``(p, axis)`` the two entries ``4 p + 2 axis +
    {0, 1}``: the two vertices of the pair's silhouette edge and the gradient in their screen
    positions, ``num_vertices`` and zeros for a slot without an active pair.  Every entry is
    written.  A ``g`` at a pixel in no active pair reaches only its own ``d``."""
    width, height = int(width), int(height)
    matrix = mesh_aa_backward_check(record, zbuf, ids, opposite, vertices, triangles, proj, color,
                                    alpha, g_color, g_alpha, width, height)
    dev = record.device
    d_color, d_alpha = torch.empty_like(color), torch.empty_like(alpha)
    entry_vertex = torch.empty((4 * width * height,), dtype=torch.int32, device=dev)
    entry_grad = torch.empty((4 * width * height, 2), dtype=torch.float32, device=dev)
    _call("ffn_mesh_aa_backward", _dev(record, torch.int32, "record"),
          _dev(zbuf, torch.int64, "zbuf"), _dev(ids, torch.int32, "ids"),
          _dev(opposite, torch.int32, "opposite"), _dev(vertices, name="vertices"),
          c_i64(vertices.shape[0]), _dev(triangles, torch.int32, "triangles"),
          c_i64(record.shape[0]), matrix, _dev(color, name="color"), _dev(alpha, name="alpha"),
          _dev(g_color, name="g_color"), _dev(g_alpha, name="g_alpha"), c_i(width), c_i(height),
          _dev(d_color), _dev(d_alpha), _dev(entry_vertex, torch.int32), _dev(entry_grad))
    return d_color, d_alpha, entry_vertex, entry_grad


def mesh_aa_vertex_grad_check(sorted_vertex, order, entry_grad, vertices, proj, grad=None,
                              accumulate: bool = False):
    """The refusals of ``mesh_aa_vertex_grad`` that need no device -> ``proj`` as 12 host
    floats."""
    who = "mesh_aa_vertex_grad"
    _raster_want(who, "entry_grad", entry_grad, torch.float32, (None, 2))
    entries = entry_grad.shape[0]
    if entries % 4 != 0 or not 1 <= entries // 4 <= MESH_AA_MAX_PIXELS:
        raise ValueError("%s: entry_grad holds %d entries; 4 per pixel of 1 .. 2^28 pixels are "
                         "supported" % (who, entries))
    _raster_want(who, "sorted_vertex", sorted_vertex, torch.int32, (entries,))
    _raster_want(who, "order", order, torch.int32, (entries,))
    _raster_want(who, "vertices", vertices, torch.float32, (None, 3))
    if not 1 <= vertices.shape[0] <= (2 ** 31 - 1) // 3:
        raise ValueError("%s: vertices holds %d vertices; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, vertices.shape[0]))
    if accumulate and grad is None:
        raise ValueError("%s: accumulate needs grad to add to" % who)
    if grad is not None:
        _raster_want(who, "grad", grad, torch.float32, (vertices.shape[0], 3))
    if np.shape(proj) != (3, 4):
        raise ValueError("%s: proj must be (3, 4), got %s" % (who, np.shape(proj)))
    return _raster_host(who, "proj", proj, 12)


def mesh_aa_vertex_grad(sorted_vertex: torch.Tensor, order: torch.Tensor,
                        entry_grad: torch.Tensor, vertices: torch.Tensor, proj,
                        grad: Optional[torch.Tensor] = None, accumulate: bool = False):
    """K34c.  ``sorted_vertex`` and ``order`` (4 H W,) int32: K34b's ``entry_vertex`` stably sorted
    and the entries in that order; ``entry_grad`` (4 H W,2) -> ``grad`` (V,3) f32: per vertex the
    sum of its entries in sorted order, put through the Jacobian of K31a's projection, a zero row
    when ``!(w > 0)``.  One thread per vertex, no atomics; the loop is linear in the vertex's run.
    ``grad`` is written in place when given, and with ``accumulate`` added to."""
    matrix = mesh_aa_vertex_grad_check(sorted_vertex, order, entry_grad, vertices, proj, grad,
                                       accumulate)
    if grad is None:
        grad = torch.empty((vertices.shape[0], 3), dtype=torch.float32, device=vertices.device)
    _call("ffn_mesh_aa_vertex_grad", _dev(sorted_vertex, torch.int32, "sorted_vertex"),
          _dev(order, torch.int32, "order"), _dev(entry_grad, name="entry_grad"),
          c_i64(entry_grad.shape[0] // 4), _dev(vertices, name="vertices"),
          c_i64(vertices.shape[0]), matrix, _dev(grad, name="grad"), c_i(1 if accumulate else 0))
    return grad


def mesh_laplacian_check(values, neighbor_starts, neighbors, scale, out=None,
                         accumulate: bool = False) -> float:
    """The refusals of ``mesh_laplacian`` that need no device -> ``scale`` as a float."""
    who = "mesh_laplacian"
    _raster_want(who, "values", values, torch.float32, (None, 3))
    if not 1 <= values.shape[0] <= (2 ** 31 - 1) // 3:
        raise ValueError("%s: values holds %d vertices; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, values.shape[0]))
    _raster_want(who, "neighbor_starts", neighbor_starts, torch.int32, (values.shape[0] + 1,))
    _raster_want(who, "neighbors", neighbors, torch.int32, (None,))
    if neighbors.shape[0] >= 2 ** 31:
        raise ValueError("%s: neighbors holds %d ids; fewer than 2^31 are supported"
                         % (who, neighbors.shape[0]))
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError("%s: scale must be finite, got %r" % (who, scale))
    if accumulate and out is None:
        raise ValueError("%s: accumulate needs out to add to" % who)
    if out is not None:
        _raster_want(who, "out", out, torch.float32, (values.shape[0], 3))
    return scale


def mesh_laplacian(values: torch.Tensor, neighbor_starts: torch.Tensor, neighbors: torch.Tensor,
                   scale: float = 1.0, out: Optional[torch.Tensor] = None,
                   accumulate: bool = False) -> torch.Tensor:
    """K34d.  ``values`` (V,3) f32 and the CSR ``neighbor_starts`` (V+1,), ``neighbors`` int32 of
    ``mesh.vertex_neighbors`` -> (V,3) f32: ``scale * sum_n (x[v] - x[n])`` over the row in order,
    ``scale`` times the gradient of ``1/2 sum_edges |x_i - x_j|^2``.  ``out`` is written in place
    when given, and with ``accumulate`` added to (``out = out + scale * acc``)."""
    scale = mesh_laplacian_check(values, neighbor_starts, neighbors, scale, out, accumulate)
    if out is None:
        out = torch.empty_like(values)
    _call("ffn_mesh_laplacian", _dev(values, name="values"),
          _dev(neighbor_starts, torch.int32, "neighbor_starts"),
          _dev(neighbors, torch.int32, "neighbors") if neighbors.numel() else _dev(None),
          c_i64(values.shape[0]), c_i64(neighbors.shape[0]), c_f(scale), _dev(out, name="out"),
          c_i(1 if accumulate else 0))
    return out


# --------------------------------------------------------------------------------- K35
def mesh_interp_face_grads_check(record, ids, d_color, colors, triangles, width: int,
                                 height: int) -> None:
    """The refusals of ``mesh_interp_face_grads`` that need no device."""
    who = "mesh_interp_face_grads"
    _raster_want(who, "triangles", triangles, torch.int32, (None, 3))
    _raster_want(who, "colors", colors, torch.float32, (None, 3))
    most = (2 ** 31 - 1) // 3
    if not 1 <= triangles.shape[0] <= most:
        raise ValueError("%s: triangles holds %d triangles; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, triangles.shape[0]))
    if not 1 <= colors.shape[0] <= most:
        raise ValueError("%s: colors holds %d vertices; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, colors.shape[0]))
    _raster_want(who, "record", record, torch.int32, (triangles.shape[0], 16))
    _raster_check_image(who, width, height)
    _raster_want(who, "ids", ids, torch.int32, (width * height,))
    _raster_want(who, "d_color", d_color, torch.float32, (width * height, 3))


def mesh_interp_face_grads(record: torch.Tensor, ids: torch.Tensor, d_color: torch.Tensor,
                           colors: torch.Tensor, triangles: torch.Tensor, width: int,
                           height: int) -> torch.Tensor:
    """K35a.  record (F,16) int32 of K31a, ids (H W,) int32 of K31c, d_color (H W,3) f32 (the
    gradient in K31c's colour; under antialiasing K34b's ``d_color``), colors (V,3) f32 and
    triangles (F,3) int32 -> ``face_grads`` (F,9) f32: per triangle, over the pixels ``ids`` gives
    it, the sums of the gradient in the screen position ``(sx, sy)`` of corner ``j`` (columns
    ``3 j``, ``3 j + 1``, in pixels) and in its ``w`` (column ``3 j + 2``) that the colour carries
    through the barycentric weights, the winner of every pixel held fixed.  K32a's organisation:
    one wavefront per triangle, a fixed order, no atomics.  A pixel whose id is another
    triangle's (or -1) is not read: a NaN there reaches nothing."""
    width, height = int(width), int(height)
    mesh_interp_face_grads_check(record, ids, d_color, colors, triangles, width, height)
    face_grads = torch.empty((record.shape[0], 9), dtype=torch.float32, device=record.device)
    _call("ffn_mesh_interp_face_grads", _dev(record, torch.int32, "record"),
          _dev(ids, torch.int32, "ids"), _dev(d_color, name="d_color"),
          _dev(colors, name="colors"), c_i64(colors.shape[0]),
          _dev(triangles, torch.int32, "triangles"), c_i64(triangles.shape[0]), c_i(width),
          c_i(height), _dev(face_grads))
    return face_grads


def mesh_interp_vertex_grad_check(face_grads, corner_order, vertex_starts, vertices, proj,
                                  grad=None, accumulate: bool = False):
    """The refusals of ``mesh_interp_vertex_grad`` that need no device -> ``proj`` as 12 host
    floats."""
    who = "mesh_interp_vertex_grad"
    _raster_want(who, "face_grads", face_grads, torch.float32, (None, 9))
    most = (2 ** 31 - 1) // 3
    if not 1 <= face_grads.shape[0] <= most:
        raise ValueError("%s: face_grads holds %d triangles; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, face_grads.shape[0]))
    _raster_want(who, "corner_order", corner_order, torch.int32, (3 * face_grads.shape[0],))
    _raster_want(who, "vertices", vertices, torch.float32, (None, 3))
    if not 1 <= vertices.shape[0] <= most:
        raise ValueError("%s: vertices holds %d vertices; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, vertices.shape[0]))
    _raster_want(who, "vertex_starts", vertex_starts, torch.int32, (vertices.shape[0] + 1,))
    if accumulate and grad is None:
        raise ValueError("%s: accumulate needs grad to add to" % who)
    if grad is not None:
        _raster_want(who, "grad", grad, torch.float32, (vertices.shape[0], 3))
    if np.shape(proj) != (3, 4):
        raise ValueError("%s: proj must be (3, 4), got %s" % (who, np.shape(proj)))
    return _raster_host(who, "proj", proj, 12)


def mesh_interp_vertex_grad(face_grads: torch.Tensor, corner_order: torch.Tensor,
                            vertex_starts: torch.Tensor, vertices: torch.Tensor, proj,
                            grad: Optional[torch.Tensor] = None, accumulate: bool = False):
    """K35b.  face_grads (F,9) of K35a, ``corner_order`` (3F,) and ``vertex_starts`` (V+1,) int32
    of ``mesh.vertex_adjacency``, vertices (V,3) f32 and ``proj`` (3,4) on the host -> ``grad``
    (V,3) f32: per vertex the sums of its corners' three columns in CSR order, put through the
    Jacobian of K31a's projection (``sx``, ``sy`` and ``w``), a zero row when ``!(w > 0)``.  One
    thread per vertex, no atomics; the loop is linear in the valence.  ``grad`` is written in
    place when given, and with ``accumulate`` added to: this is how it joins K34c's result."""
    matrix = mesh_interp_vertex_grad_check(face_grads, corner_order, vertex_starts, vertices, proj,
                                           grad, accumulate)
    if grad is None:
        grad = torch.empty((vertices.shape[0], 3), dtype=torch.float32, device=vertices.device)
    _call("ffn_mesh_interp_vertex_grad", _dev(face_grads, name="face_grads"),
          _dev(corner_order, torch.int32, "corner_order"),
          _dev(vertex_starts, torch.int32, "vertex_starts"), c_i64(face_grads.shape[0]),
          _dev(vertices, name="vertices"), c_i64(vertices.shape[0]), matrix,
          _dev(grad, name="grad"), c_i(1 if accumulate else 0))
    return grad


# --------------------------------------------------------------------------------- K36
MESH_CAST_MAX_LEAF = 64
MESH_CAST_MAX_LEVELS = 31
MESH_CAST_MAX_RAYS = 2 ** 31 - 1
MESH_CAST_EMPTY_KEY = 1 << 30       # K36a's key of a triangle with a non-finite vertex


def mesh_cast_levels(num_triangles: int, leaf_size: int) -> int:
    """The levels of K36's tree: the smallest count whose ``2^(levels - 1)`` leaves of
    ``leaf_size`` triangles hold every triangle."""
    levels = 1
    while (leaf_size << (levels - 1)) < num_triangles:
        levels += 1
    return levels


def _cast_number(who, name, value, low=None):
    if isinstance(value, bool) or not isinstance(value, numbers.Real) \
            or not math.isfinite(value) or (low is not None and value < low):
        raise ValueError("%s: %s must be a finite number%s, got %r"
                         % (who, name, "" if low is None else " >= %g" % low, value))
    return float(value)


def _cast_check_tree(who, boxes, order, leaf_size, nodes=None, with_nodes=False) -> int:
    """boxes (F,6), order (F,), ``leaf_size`` and, ``with_nodes``, nodes (2^levels - 1, 6) ->
    levels."""
    _raster_want(who, "boxes", boxes, torch.float32, (None, 6))
    num = boxes.shape[0]
    if not 1 <= num <= (2 ** 31 - 1) // 3:
        raise ValueError("%s: boxes holds %d triangles; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, num))
    _raster_want(who, "order", order, torch.int32, (num,))
    _want_int(who, "leaf_size", leaf_size, 1, MESH_CAST_MAX_LEAF)
    levels = mesh_cast_levels(num, leaf_size)
    if levels > MESH_CAST_MAX_LEVELS:
        raise ValueError("%s: boxes and leaf_size need %d levels; at most %d are supported"
                         % (who, levels, MESH_CAST_MAX_LEVELS))
    if with_nodes:
        _raster_want(who, "nodes", nodes, torch.float32, ((1 << levels) - 1, 6))
    return levels


def mesh_cast_boxes_check(vertices, triangles, pad, grid_lo, grid_scale):
    """The refusals of ``mesh_cast_boxes`` that need no device -> (pad, grid_lo, grid_scale) as
    host floats."""
    who = "mesh_cast_boxes"
    _raster_check_mesh(who, vertices, triangles)
    pad = _cast_number(who, "pad", pad, 0.0)
    scale = _cast_number(who, "grid_scale", grid_scale, 0.0)
    corner = np.asarray(grid_lo, dtype=np.float64).reshape(-1)
    if corner.shape != (3,) or not np.isfinite(corner).all():
        raise ValueError("%s: grid_lo must be three finite numbers, got %r" % (who, grid_lo))
    return pad, [float(c) for c in corner], scale


def mesh_cast_boxes(vertices: torch.Tensor, triangles: torch.Tensor, pad: float, grid_lo,
                    grid_scale: float):
    """K36a.  vertices (V,3) f32, triangles (F,3) int32 (ids clamped into the vertices) ->
    ``(boxes (F,6) f32, keys (F,) int32)``: per triangle ``min(a,b,c) - pad`` and ``max(a,b,c) +
    pad`` (the empty box ``+inf, -inf`` when a coordinate is not finite) and the 30-bit Morton code
    of the box centre on the grid of 1024 cells a side that starts at ``grid_lo`` with
    ``grid_scale`` cells per unit (``MESH_CAST_EMPTY_KEY`` for an empty box)."""
    pad, corner, scale = mesh_cast_boxes_check(vertices, triangles, pad, grid_lo, grid_scale)
    num = triangles.shape[0]
    boxes = torch.empty((num, 6), dtype=torch.float32, device=vertices.device)
    keys = torch.empty((num,), dtype=torch.int32, device=vertices.device)
    _call("ffn_mesh_cast_boxes", _dev(vertices, name="vertices"), c_i64(vertices.shape[0]),
          _dev(triangles, torch.int32, "triangles"), c_i64(num), c_f(pad), c_f(corner[0]),
          c_f(corner[1]), c_f(corner[2]), c_f(scale), _dev(boxes), _dev(keys, torch.int32))
    return boxes, keys


def mesh_cast_tree_check(boxes, order, leaf_size) -> int:
    """The refusals of ``mesh_cast_tree`` that need no device -> the number of levels."""
    return _cast_check_tree("mesh_cast_tree", boxes, order, leaf_size)


def mesh_cast_tree(boxes: torch.Tensor, order: torch.Tensor, leaf_size: int) -> torch.Tensor:
    """K36b.  boxes (F,6) f32 of K36a, order (F,) int32 (a permutation of the triangles; entries
    are clamped) -> ``nodes`` (2^levels - 1, 6) f32, ``levels = mesh_cast_levels(F, leaf_size)``:
    the boxes of the complete binary tree whose leaf ``j`` holds the triangles
    ``order[j leaf_size : (j + 1) leaf_size]``, level ``l`` from row ``2^l - 1``; the empty box for
    a node over no triangle."""
    levels = mesh_cast_tree_check(boxes, order, leaf_size)
    nodes = torch.empty(((1 << levels) - 1, 6), dtype=torch.float32, device=boxes.device)
    _call("ffn_mesh_cast_tree", _dev(boxes, name="boxes"), _dev(order, torch.int32, "order"),
          c_i64(boxes.shape[0]), c_i(leaf_size), c_i(levels), _dev(nodes))
    return nodes


def mesh_cast_check(nodes, boxes, order, vertices, triangles, starts, directions, leaf_size,
                    t_min=0.0, farthest: bool = False):
    """The refusals of ``mesh_cast`` that need no device -> (levels, t_min)."""
    who = "mesh_cast"
    _raster_check_mesh(who, vertices, triangles)
    _raster_want(who, "boxes", boxes, torch.float32, (triangles.shape[0], 6))
    levels = _cast_check_tree(who, boxes, order, leaf_size, nodes, True)
    _raster_want(who, "starts", starts, torch.float32, (None, 3))
    if not 1 <= starts.shape[0] <= MESH_CAST_MAX_RAYS:
        raise ValueError("%s: starts holds %d rays; 1 .. 2^31 - 1 are supported"
                         % (who, starts.shape[0]))
    _raster_want(who, "directions", directions, torch.float32, (starts.shape[0], 3))
    if isinstance(t_min, bool) or not isinstance(t_min, numbers.Real) or math.isnan(t_min):
        raise ValueError("%s: t_min must be a number, not NaN, got %r" % (who, t_min))
    return levels, float(t_min)


def mesh_cast(nodes: torch.Tensor, boxes: torch.Tensor, order: torch.Tensor,
              vertices: torch.Tensor, triangles: torch.Tensor, starts: torch.Tensor,
              directions: torch.Tensor, leaf_size: int, t_min: float = 0.0,
              farthest: bool = False):
    """K36c.  nodes, boxes, order of K36a/b, the mesh they were built from, starts and directions
    (R,3) f32 -> ``(hit (R,) int32, t, u, v (R,) f32)``: per ray the triangle with the least
    ``(t, id)`` among those it hits beyond ``t_min`` (with ``farthest`` the greatest ``t``, ties to
    the lower id) and Moeller-Trumbore's ``t, u, v`` of that hit; -1 and zeros for a miss.  Two-sided;
    a ray in a triangle's plane, and a NaN or infinite ray, misses.  One lane per ray, a stackless
    walk with a trip bound; no atomics, no LDS, no scratch."""
    levels, t_min = mesh_cast_check(nodes, boxes, order, vertices, triangles, starts, directions,
                                    leaf_size, t_min, farthest)
    dev, num = starts.device, starts.shape[0]
    hit = torch.empty((num,), dtype=torch.int32, device=dev)
    t, u, v = (torch.empty((num,), dtype=torch.float32, device=dev) for _ in range(3))
    _call("ffn_mesh_cast", _dev(nodes, name="nodes"), _dev(boxes, name="boxes"),
          _dev(order, torch.int32, "order"), _dev(vertices, name="vertices"),
          c_i64(vertices.shape[0]), _dev(triangles, torch.int32, "triangles"),
          c_i64(triangles.shape[0]), c_i(leaf_size), c_i(levels), _dev(starts, name="starts"),
          _dev(directions, name="directions"), c_i64(num), c_f(t_min), c_i(1 if farthest else 0),
          _dev(hit, torch.int32), _dev(t), _dev(u), _dev(v))
    return hit, t, u, v


def mesh_cast_shade_check(hit, t, u, v, triangles, colors, uvs, texture, background):
    """The refusals of ``mesh_cast_shade`` that need no device -> (number of vertices, background
    as three host floats).  Exactly one of ``colors`` and ``uvs`` + ``texture`` is given."""
    who = "mesh_cast_shade"
    _raster_want(who, "hit", hit, torch.int32, (None,))
    num = hit.shape[0]
    if not 1 <= num <= MESH_CAST_MAX_RAYS:
        raise ValueError("%s: hit holds %d rays; 1 .. 2^31 - 1 are supported" % (who, num))
    for name, value in (("t", t), ("u", u), ("v", v)):
        _raster_want(who, name, value, torch.float32, (num,))
    _raster_want(who, "triangles", triangles, torch.int32, (None, 3))
    most = (2 ** 31 - 1) // 3
    if not 1 <= triangles.shape[0] <= most:
        raise ValueError("%s: triangles holds %d triangles; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, triangles.shape[0]))
    if (colors is None) == (uvs is None and texture is None) or (uvs is None) != (texture is None):
        raise ValueError("%s: give either colors, or uvs and texture" % who)
    if colors is not None:
        _raster_want(who, "colors", colors, torch.float32, (None, 3))
        vertices = colors.shape[0]
    else:
        _raster_want(who, "uvs", uvs, torch.float32, (None, 2))
        vertices = uvs.shape[0]
        _raster_want(who, "texture", texture, torch.uint8, (None, None, None))
        tex_h, tex_w, channels = texture.shape
        if (channels < 3 or not 1 <= tex_h <= MESH_MAX_TEXTURE_SIDE
                or not 1 <= tex_w <= MESH_MAX_TEXTURE_SIDE or tex_h * tex_w * channels >= 2 ** 31):
            raise ValueError("%s: texture must be (H, W, C) with C >= 3, 1 <= H, W <= 2^24 and "
                             "fewer than 2^31 bytes, got %s" % (who, tuple(texture.shape)))
    if not 1 <= vertices <= most:
        raise ValueError("%s: %s holds %d vertices; 1 .. (2^31 - 1) / 3 are supported"
                         % (who, "colors" if colors is not None else "uvs", vertices))
    ground = np.asarray(background, dtype=np.float32).reshape(-1)
    if ground.shape != (3,) or not np.isfinite(ground).all():
        raise ValueError("%s: background must be 3 finite numbers, got %r" % (who, background))
    return vertices, [float(c) for c in ground]


def mesh_cast_shade(hit: torch.Tensor, t: torch.Tensor, u: torch.Tensor, v: torch.Tensor,
                    triangles: torch.Tensor, colors: Optional[torch.Tensor],
                    uvs: Optional[torch.Tensor], texture: Optional[torch.Tensor],
                    background=(0.0, 0.0, 0.0)):
    """K36d.  hit, t, u, v (R,) of K36c and the mesh's triangles (F,3) int32 -> ``(color (R,3),
    alpha (R,), depth (R,))`` f32: the hit triangle's ``colors`` (V,3) under the weights ``(1 - u)
    - v, u, v``, or its ``uvs`` (V,2) under them through ``texture`` (h,w,C) uint8 with the row
    index growing with ``v`` (K22's lookup); 1; ``t``.  A miss gets ``background``, 0 and 0."""
    vertices, ground = mesh_cast_shade_check(hit, t, u, v, triangles, colors, uvs, texture,
                                             background)
    dev, num = hit.device, hit.shape[0]
    color = torch.empty((num, 3), dtype=torch.float32, device=dev)
    alpha = torch.empty((num,), dtype=torch.float32, device=dev)
    depth = torch.empty((num,), dtype=torch.float32, device=dev)
    tex_h, tex_w, channels = (0, 0, 0) if texture is None else texture.shape
    _call("ffn_mesh_cast_shade", _dev(hit, torch.int32, "hit"), _dev(t, name="t"),
          _dev(u, name="u"), _dev(v, name="v"), c_i64(num),
          _dev(triangles, torch.int32, "triangles"), c_i64(triangles.shape[0]),
          _dev(colors, name="colors"), _dev(uvs, name="uvs"), c_i64(vertices),
          _dev(texture, torch.uint8, "texture"), c_i(tex_h), c_i(tex_w), c_i(channels),
          c_f(ground[0]), c_f(ground[1]), c_f(ground[2]), _dev(color), _dev(alpha), _dev(depth))
    return color, alpha, depth
