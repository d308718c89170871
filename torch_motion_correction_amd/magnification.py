"""Anisotropic magnification distortion correction of sums and stacks (mc_affine_resample, csrc/affine_resample.hip
over csrc/affine_resample.h): what MotionCor2's ``-Mag major minor angle``, cisTEM / Unblur and RELION do at this stage.

THE CONVENTION.  The distortion stretches the image by ``major_scale`` along the direction at ``major_axis_angle``
degrees, measured from +x (columns) towards +y (rows) of the array, and by ``minor_scale`` across it.  With
u = (cos, sin) of that angle as (x, y) components, D = major_scale * u u^T + minor_scale * (I - u u^T) in (x, y) order;
the corrected image samples the distorted one at c + D (p - c), c = (h // 2, w // 2), so that content stretched by
``major_scale`` along the angle returns to scale 1.  M is D rewritten in (y, x) order.  This is the package's OWN sign
and angle convention: it has not been checked against output of MotionCor2 or cisTEM, none of which was available where
this was written.  The resampling rule itself is stated once, in csrc/affine_resample.h.

THE ALIGNED SUM IN ONE RESAMPLING.  ``motion_correct_sum_magnified`` and ``motion_correct_sum_magnified_raw``
(mc_affine_warp_sum, csrc/affine_warp_sum.hip over csrc/affine_warp_sum.h) fold M into the rigid warp: frame f is
sampled once, at c + M (p - c) + shift_f, and the frames are added as they are formed -- one interpolation instead of
the rigid warp's followed by ``correct_magnification_distortion``'s, and for a raw uint8 / int16 movie no conditioned
fp32 copy of it.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib, engine
from ._lib import check, gpu_entry, ptr, stream_ptr
from ._lib import require_gpu  # noqa: F401  (unused here; tests/test_magnification_host.py patches this name)

SCALE_MIN, SCALE_MAX = 0.9, 1.1  # of major_scale and minor_scale; bounds the source footprint of an output tile


def _real(value, name):
    """A finite real number (no bool, no tensor-likes that float() refuses) -> float; ValueError otherwise."""
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a finite real number, got {value!r}")
    v = float(value)
    if not math.isfinite(v):
        raise ValueError(f"{name} must be a finite real number, got {value!r}")
    return v


def _check_parameters(major_scale, minor_scale, major_axis_angle):
    major, minor = _real(major_scale, "major_scale"), _real(minor_scale, "minor_scale")
    angle = _real(major_axis_angle, "major_axis_angle")
    for name, v in (("major_scale", major), ("minor_scale", minor)):
        if not SCALE_MIN <= v <= SCALE_MAX:
            raise ValueError(f"{name} must lie in [{SCALE_MIN}, {SCALE_MAX}], got {v!r}")
    return major, minor, angle


def magnification_distortion_matrix(major_scale, minor_scale, major_axis_angle):
    """The (2, 2) float64 matrix M, in (y, x) order, that ``correct_magnification_distortion`` resamples through:
    output pixel p samples the input at c + M (p - c), c = (h // 2, w // 2).  Host only.

    ``major_scale``, ``minor_scale``: the distortion's magnification along and across the major axis, each in
    [0.9, 1.1].  ``major_axis_angle``: degrees from +x (columns) towards +y (rows) of the array.  In (x, y) order
    D = major_scale * u u^T + minor_scale * (I - u u^T) with u = (cos, sin) of the angle; M is D with its axes
    swapped: M[0, 0] = D_yy, M[0, 1] = M[1, 0] = D_xy, M[1, 1] = D_xx.  The angle and the angle + 180 degrees, and
    (major, minor, angle) and (minor, major, angle + 90 degrees), give the same matrix.  This is the package's own
    sign and angle convention, not checked against MotionCor2 or cisTEM output (none was available).

    A bool, a value that is not a finite real number and a scale outside [0.9, 1.1] raise ValueError naming the
    argument."""
    major, minor, angle = _check_parameters(major_scale, minor_scale, major_axis_angle)
    # u u^T from cos(2 a), sin(2 a) of the angle reduced into (-180, 180): a and a + 180 reduce to the same value, and
    # at a = 0 the products below are exactly 1, 0, 0, so that axis' scale alone changes and the other stays `minor`
    a2 = math.radians(2.0 * math.fmod(angle, 180.0))
    c2, s2 = math.cos(a2), math.sin(a2)
    cc, ss, sc = 0.5 * (1.0 + c2), 0.5 * (1.0 - c2), 0.5 * s2
    d = major - minor
    # D = minor I + (major - minor) u u^T in (x, y) order
    dxx, dyy, dxy = minor + d * cc, minor + d * ss, d * sc
    return torch.tensor([[dyy, dxy], [dxy, dxx]], dtype=torch.float64)


def _check_image(image):
    if not isinstance(image, torch.Tensor) or image.dim() not in (2, 3) or \
            image.dtype not in (torch.float32, torch.float16):
        raise ValueError("image must be an (h, w) or (t, h, w) tensor of dtype float32 or float16, got "
                         f"{getattr(image, 'dtype', type(image).__name__)} {tuple(getattr(image, 'shape', ()))}")
    if image.numel() == 0:
        raise ValueError(f"image must not be empty, got shape {tuple(image.shape)}")
    h, w = image.shape[-2:]
    if h < 4 or w < 4:
        raise ValueError(f"image must have at least 4 rows and 4 columns, got shape {tuple(image.shape)}")
    if h * w >= 2**31:
        raise ValueError(f"image shape {tuple(image.shape)}: frames of 2^31 samples and more are not supported")


def _resample(src, matrix, fill_value, out=None):
    """The (t, h, w) stack `src` on the current GPU through mc_affine_resample -> (t, h, w) fp32, in chunks of frames
    by the workspace rule (engine._chunks over an output frame's bytes).  Chunks are independent: the result does not
    depend on their size.  `out`: the buffer to write (the tests' guarded buffers)."""
    lib = _lib.load()
    t, h, w = src.shape
    if out is None:
        out = torch.empty((t, h, w), dtype=torch.float32, device=src.device)
    assert out.dtype == torch.float32 and out.shape == src.shape and out.device == src.device and out.is_contiguous()
    m = (C.c_double * 4)(*(float(v) for v in matrix.reshape(-1).tolist()))
    _, spans = engine._chunks(t, h * w * 4)
    for a, n in spans:
        check(lib.mc_affine_resample(ptr(src[a:a + n]), engine.storage_of(src), n, h, w, m, fill_value,
                                     ptr(out[a:a + n]), stream_ptr(src.device)), "mc_affine_resample")
    return out


def correct_magnification_distortion(image, major_scale, minor_scale, major_axis_angle, fill_value=0.0, device=None):
    """A sum ``(h, w)`` or a stack ``(t, h, w)`` with the microscope's anisotropic magnification distortion removed
    -> float32 of the same shape.  Correct the sums, or the aligned stack, after motion correction and before CTF
    estimation.

    ``image``: float32 or float16 (read from its bytes; the result is that of the up-cast input, bit for bit), CPU or
    GPU, h, w >= 4.  ``major_scale``, ``minor_scale``, ``major_axis_angle``: the distortion as
    ``magnification_distortion_matrix`` takes it -- the magnification along and across the major axis, each in
    [0.9, 1.1], and the axis' angle in degrees from +x towards +y of the array; the package's own convention, not
    checked against MotionCor2 or cisTEM output.  Output pixel p is the input sampled at c + M (p - c),
    c = (h // 2, w // 2): the position in float64 on the device, 4 x 4 bicubic (Keys, A = -0.75, the weights of the
    package's warps) in fp32 with taps beyond the edge clamped to it; a position outside [0, h - 1] x [0, w - 1]
    gives ``fill_value`` (csrc/affine_resample.h states the rule).  Scales of 1 still run the kernel and return the
    input's values exactly.  Frames are independent; a stack beyond the engine's workspace rule goes through in
    chunks of frames, with the same result.

    The result is on ``device`` if given, else on the device of ``image``; a CPU image is staged to the current GPU
    and the result copied back.  There is no CPU fallback.  Every argument rule -- a bool or a value that is not a
    finite real number for a parameter or ``fill_value``, a scale outside [0.9, 1.1], an ``image`` that is not a 2-
    or 3-dimensional float32 / float16 tensor -- is a ValueError naming the argument, raised before any device is
    touched."""
    _check_image(image)
    matrix = magnification_distortion_matrix(major_scale, minor_scale, major_axis_angle)
    fill_value = _real(fill_value, "fill_value")
    with gpu_entry(image, device) as (out_dev, dev):
        src = image.detach().to(dev).contiguous()
        out = _resample(src if src.dim() == 3 else src[None], matrix, fill_value)
        return (out if image.dim() == 3 else out[0]).to(out_dev)


# ------------------------------------------------------------------ the aligned sum with M folded into the rigid warp


def _check_stack(stack, name, dtypes, names):
    if not isinstance(stack, torch.Tensor) or stack.dim() != 3 or stack.dtype not in dtypes:
        raise ValueError(f"{name} must be a (t, h, w) tensor of dtype {names}, got "
                         f"{getattr(stack, 'dtype', type(stack).__name__)} {tuple(getattr(stack, 'shape', ()))}")
    if stack.numel() == 0:
        raise ValueError(f"{name} must not be empty, got shape {tuple(stack.shape)}")
    h, w = stack.shape[-2:]
    if h < 4 or w < 4:
        raise ValueError(f"{name} must have at least 4 rows and 4 columns, got shape {tuple(stack.shape)}")
    if h * w >= 2**31:
        raise ValueError(f"{name} shape {tuple(stack.shape)}: frames of 2^31 samples and more are not supported")


def _pixel_shifts(deformation_grid, t, pixel_spacing):
    """The (t, 2) fp32 pixel shifts (y, x), on the CPU, of a rigid (2, t, 1, 1) Angstrom field with one node per frame:
    the correctly rounded fp32 quotient fp32(L) / fp32(ps), true division of a CPU tensor by an fp32 tensor (the
    canonical rule of the rigid warp; a multiply by the fp32 reciprocal is one ulp off for some shifts).  Every rule
    of the field and of the spacing is a ValueError."""
    field = deformation_grid
    if not isinstance(field, torch.Tensor) or field.dim() != 4 or field.shape[0] != 2 or min(field.shape) < 1:
        raise ValueError(f"deformation_grid must be a (2, t, 1, 1) tensor, got {tuple(getattr(field, 'shape', ()))}")
    if tuple(field.shape[-2:]) != (1, 1):
        raise ValueError(f"deformation_grid must be a rigid (2, t, 1, 1) field, one shift per frame, got shape "
                         f"{tuple(field.shape)}: a local field (more than one patch) is not supported by the "
                         "magnified sum")
    if field.shape[1] != t:
        raise ValueError(f"deformation_grid has {field.shape[1]} time points, the movie {t} frames")
    if not field.dtype.is_floating_point:
        raise ValueError(f"deformation_grid must be a floating-point tensor, got {field.dtype}")
    ps = _real(pixel_spacing, "pixel_spacing")
    if not ps > 0.0:
        raise ValueError(f"pixel_spacing must be > 0, got {pixel_spacing!r}")
    lattice = field.detach()[:, :, 0, 0].to(device="cpu", dtype=torch.float32)
    if not bool(torch.isfinite(lattice).all()):
        raise ValueError("deformation_grid must be finite: it holds a value that is not a finite number")
    shifts = torch.div(lattice, torch.tensor(ps, dtype=torch.float32))
    if not bool(torch.isfinite(shifts).all()):
        raise ValueError(f"deformation_grid / pixel_spacing overflows fp32 (pixel_spacing {ps!r})")
    return shifts.t().contiguous()


def _warp_sum(src, kind, gain, mu, matrix, shifts, want_frames, out=None):
    """mc_affine_warp_sum on the current GPU: `src` (t, h, w) of storage `kind` there, `gain` / `mu` for the raw
    kinds, `shifts` (t, 2) fp32 on the CPU -> (sum (h, w) fp32, frames (t, h, w) fp32 or None).  `out`: the
    (sum, frames or None) buffers to write (the tests' guarded buffers)."""
    lib = _lib.load()
    t, h, w = src.shape
    dev = src.device
    total, frames = out if out is not None else (
        torch.empty((h, w), dtype=torch.float32, device=dev),
        torch.empty((t, h, w), dtype=torch.float32, device=dev) if want_frames else None)
    m = (C.c_double * 4)(*(float(v) for v in matrix.reshape(-1).tolist()))
    sh = shifts.to(dev)
    check(lib.mc_affine_warp_sum(ptr(src), kind, ptr(gain), ptr(mu), t, h, w, m, ptr(sh), ptr(total), ptr(frames),
                                 stream_ptr(dev)), "mc_affine_warp_sum")
    return total, frames


def motion_correct_sum_magnified(image, deformation_grid, pixel_spacing, major_scale, minor_scale, major_axis_angle,
                                 return_frames=False, device=None):
    """The aligned sum of a movie with the magnification distortion removed, each frame interpolated ONCE -> the
    ``(h, w)`` float32 sum, or ``(sum, frames (t, h, w))`` with ``return_frames``.

    What ``correct_magnification_distortion(motion_correct_sum(image, ...), ...)`` does with two bicubic passes (the
    rigid warp, then the 2 x 2 map) is done here with one: output pixel p of frame f samples it at
    c + M (p - c) + s_f, c = (h // 2, w // 2), in float64 on the device, with the 4 x 4 Keys weights of
    ``correct_magnification_distortion`` in fp32 and taps beyond the edge clamped to it; a position outside
    [0, h - 1] x [0, w - 1] contributes exactly 0, the rigid warp's rule (there is no ``fill_value``).  The sum is the
    fp32 sequence ((0 + v_0) + v_1) + ... in frame order, one accumulator per pixel: its bits do not depend on the
    launch.  csrc/affine_warp_sum.h states the rule.

    ``image``: a (t, h, w) float32 or float16 stack (fp16 is read from its bytes; the result is that of the up-cast
    input, bit for bit), CPU or GPU, h, w >= 4.  ``deformation_grid``: a rigid (2, t, 1, 1) field in Angstrom with one
    node per frame, (y, x) as for ``motion_correct_sum``; the pixel shift is the correctly rounded fp32 quotient
    ``fp32(field) / fp32(pixel_spacing)`` and, as in the rigid warp, a sample is taken at p + s.  A local field
    (more than one patch) is a ValueError: the general-field warp with M folded in is not built.  ``major_scale``,
    ``minor_scale``, ``major_axis_angle``: as ``magnification_distortion_matrix`` takes them (the package's own
    convention).

    There is no hot-pixel step and no dose weighting here: a dose-weighted sum needs a transform per frame.  The
    result is on ``device`` if given, else on the device of ``image``; a CPU image is staged to the current GPU and
    the result copied back.  There is no CPU fallback.  Every argument rule is a ValueError raised before any device
    is touched."""
    _check_stack(image, "image", (torch.float32, torch.float16), "float32 or float16")
    shifts = _pixel_shifts(deformation_grid, image.shape[0], pixel_spacing)
    matrix = magnification_distortion_matrix(major_scale, minor_scale, major_axis_angle)
    want_frames = bool(return_frames)
    with gpu_entry(image, device) as (out_dev, dev):
        src = image.detach().to(dev).contiguous()
        total, frames = _warp_sum(src, engine.storage_of(src), None, None, matrix, shifts, want_frames)
        return (total.to(out_dev), frames.to(out_dev)) if want_frames else total.to(out_dev)


def motion_correct_sum_magnified_raw(movie, gain, deformation_grid, pixel_spacing, major_scale, minor_scale,
                                     major_axis_angle, mean_zero=True, return_frames=False, device=None):
    """``motion_correct_sum_magnified(condition_movie(movie, gain, mean_zero), ...)`` for a RAW uint8 / int16 movie,
    without the conditioned fp32 movie: one statistics pass (engine.RawMovie) gives the frame means, and the kernel
    forms ``fp32(raw) * gain - frame mean`` as ``condition_movie`` rounds it (product and difference rounded
    separately) on its way into the resampler's window, once per sample.  With the frame means of that pass equal to
    ``condition_movie``'s -- always without ``mean_zero``; with it, wherever both kernels sum a frame in the same
    order (w % 8 == 0) -- the result is that composition's bit for bit.

    ``movie``: (t, h, w) uint8 or int16, CPU or GPU; ``gain``: (h, w), or None for ones.  Every other argument, the
    sampling rule and the result are ``motion_correct_sum_magnified``'s.  There is no hot-pixel step and no dose
    weighting here; there is no CPU fallback; every argument rule is a ValueError raised before any device is
    touched."""
    _check_stack(movie, "movie", (torch.uint8, torch.int16), "uint8 or int16")
    if gain is not None and (not isinstance(gain, torch.Tensor) or tuple(gain.shape) != tuple(movie.shape[-2:])):
        raise ValueError(f"gain reference has shape {tuple(getattr(gain, 'shape', ()))}, frames are "
                         f"{tuple(movie.shape[-2:])}")
    shifts = _pixel_shifts(deformation_grid, movie.shape[0], pixel_spacing)
    matrix = magnification_distortion_matrix(major_scale, minor_scale, major_axis_angle)
    want_frames = bool(return_frames)
    with gpu_entry(movie, device) as (out_dev, dev):
        rm = engine.RawMovie(movie.detach().to(dev), None if gain is None else gain.detach().to(dev),
                             mean_zero=bool(mean_zero))
        total, frames = _warp_sum(rm.raw, rm.kind, rm.gain, rm.mu, matrix, shifts, want_frames)
        return (total.to(out_dev), frames.to(out_dev)) if want_frames else total.to(out_dev)
