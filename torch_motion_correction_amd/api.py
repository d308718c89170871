"""Reference-compatible Python entry points (same names, argument order, defaults,
shapes, units and error behaviour as torch_motion_correction's public API,
src/torch_motion_correction/__init__.py:12-44), executing on the MI355X through
libmcorr.  No CPU fallback exists: without a ROCm device these raise McorrError.

Device rule (reference: ``device=None`` -> ``image.device``): results are returned on
the device the reference would have returned them on; when that device is the CPU,
inputs are staged to the current GPU, computed there and copied back.

``BUG_COMPATIBLE`` (default True) keeps the reference's behavioural accidents that
change numbers or mutate arguments: the in-place negation of
the caller's field in ``correct_motion_fast`` (Q1) and the mask-exponent schedule
caused by the lazy-patch memo aliasing (Q2/Q3), and the RuntimeError the reference raises
for sub_pixel_refinement=False with outlier_rejection=True (Q12: torch.std on int64
peaks).  Q4-Q9 are plain semantics and are always reproduced.
"""

from __future__ import annotations

import math
import operator

import torch

from . import engine
from ._lib import McorrUnsupported, gpu_entry, normalize_frame_index, say
from ._lib import device_scope, require_gpu  # noqa: F401  (unused here; host tests patch these names on `api`)

BUG_COMPATIBLE = True
RIGID_FAST_PATH = True  # (2,nt,1,1) fields use the separable rigid warp kernel
VERBOSE = False  # the reference prints progress lines (_lib.say); opt in with VERBOSE = True


def _is_rigid(field: torch.Tensor) -> bool:
    return tuple(field.shape[-2:]) == (1, 1)


def _stage(x: torch.Tensor, dev, keep_half: bool = False) -> torch.Tensor:
    """The tensor on the GPU as contiguous fp32 -- or, `keep_half`, an fp16 stack as it is: the patch
    estimator and the deformation-field warp read fp16 frames straight from their bytes (BASELINE
    C5; no fp32 copy of the movie, half the HBM read)."""
    if keep_half and x.dtype == torch.float16:
        return x.detach().to(device=dev).contiguous()
    return x.detach().to(device=dev, dtype=torch.float32).contiguous()


# Every entry point computes under ``with gpu_entry(first, device) as (out_dev, dev):`` (_lib): libmcorr launches on
# the current HIP device, the reference takes ``device=`` / the first tensor's device per call.  Where a function has
# argument rules of its own that are promised "before any device is touched", they stand before the ``with``; every
# other function opens with it, and so needs a GPU before its body refuses anything.

# ------------------------------------------------------------------ raw movies: one route
RAW_DTYPES = (torch.uint8, torch.int16)  # storage the fused kernels (engine.RawMovie) read


def _stage_raw(movie, gain, dev):
    """Staging of every raw entry point -> (the movie on the GPU `dev` in its own storage type, the gain there or
    None)."""
    return movie.detach().to(dev), None if gain is None else gain.to(dev)


def _raw_or_conditioned(raw, gd, mean_zero, thr, fused, conditioned, allow_fused=True):
    """THE fused-or-conditioned rule of the raw entry points -> (result, (t,) int32 hot counts or None).
    A u8 / i16 movie (and `allow_fused`, the caller's own preconditions) goes through ONE engine.RawMovie:
    ``fused(rm)``, with the RawMovie's counts.  Where its constructor or `fused` raises McorrUnsupported (a shape
    without a fused kernel, a hot-pixel list overflow) -- nothing else is caught -- and for every other movie, the
    route is exactly ``conditioned(engine.condition_movie(raw, gd, mean_zero, thr))``.  The counts are asked of
    condition_movie whenever a threshold is set: it enqueues the same kernel into the same buffers either way
    (mc_condition_movie_hot always writes them), so callers that drop them launch what they did before."""
    if allow_fused and raw.dtype in RAW_DTYPES:
        try:
            rm = engine.RawMovie(raw, gd, mean_zero=bool(mean_zero), hot_pixel_threshold=thr)
            return fused(rm), rm.hot_counts
        except McorrUnsupported:
            pass
    img, counts = engine.condition_movie(raw, gd, bool(mean_zero), hot_pixel_threshold=thr,
                                         return_hot_counts=thr is not None), None
    if thr is not None:
        img, counts = img
    return conditioned(img), counts


def _hot_counts_out(counts, t, out_dev):
    """The ``return_hot_counts`` result: zeros where no threshold was set."""
    return torch.zeros(t, dtype=torch.int32, device=out_dev) if counts is None else counts.to(out_dev)


def _check_patch_sidelength(patch_sidelength, frame=None):
    """The patch side as an int > 0 (ValueError).  With `frame` (h, w) -- the refinements' rules -- a value int()
    refuses is a ValueError of ours too, and the patch has to fit the frame."""
    try:
        p = int(patch_sidelength)
    except (TypeError, ValueError):
        if frame is None:
            raise
        raise ValueError(f"patch_sidelength must be an integer > 0, got {patch_sidelength!r}") from None
    if not p > 0:
        raise ValueError(f"patch_sidelength must be > 0, got {patch_sidelength!r}")
    if frame is not None and (p > frame[0] or p > frame[1]):
        raise ValueError(f"patch_sidelength {p} exceeds the frame size {frame[0]}x{frame[1]}")
    return p


def _check_field_4d(field, what):
    """A (2, nt, gh, gw) tensor without an empty axis; ValueError opening with `what` otherwise."""
    if not isinstance(field, torch.Tensor) or field.dim() != 4 or field.shape[0] != 2 or min(field.shape) < 1:
        raise ValueError(f"{what}, got {tuple(getattr(field, 'shape', ()))}")


# ------------------------------------------------------------------ field utilities


def image_shifts_to_deformation_field(shifts, pixel_spacing, device=None):
    """(t,2) px shifts -> (2,t,1,1) Angstrom field, no sign flip
    (deformation_field_utils.py:129-162)."""
    if device is not None:
        shifts = shifts.to(device)
    return (shifts * pixel_spacing).transpose(0, 1)[:, :, None, None]


def evaluate_deformation_field(deformation_field, tyx, grid_type="catmull_rom"):
    """(c,nt,nh,nw) spline grid evaluated at (...,3) tyx points in [0,1] -> (...,c)
    (deformation_field_utils.py:9-39): one launch over all points (mc_spline_points)."""
    with gpu_entry(deformation_field) as (out_dev, dev):
        field = _stage(deformation_field, dev)
        vals = engine.spline_points(field, tyx.reshape(-1, 3), grid_type)
        return vals.reshape(*tyx.shape[:-1], field.shape[0]).to(out_dev)


def evaluate_deformation_field_at_t(deformation_field, t, grid_shape, grid_type="catmull_rom"):
    """(c, H, W) shifts on the linspace(0,1) lattice at time t
    (deformation_field_utils.py:42-93)."""
    with gpu_entry(deformation_field) as (out_dev, dev):
        H, W = grid_shape
        lat = engine.spline_lattice(_stage(deformation_field, dev),
                                    torch.as_tensor([float(t)], dtype=torch.float32),
                                    torch.linspace(0, 1, steps=H), torch.linspace(0, 1, steps=W), grid_type)
        return lat[:, 0].to(out_dev)


def resample_deformation_field(deformation_field, target_resolution):
    """Catmull-Rom resample to (nt,nh,nw) (deformation_field_utils.py:96-126)."""
    with gpu_entry(deformation_field) as (out_dev, dev):
        nt, nh, nw = target_resolution
        lat = engine.spline_lattice(_stage(deformation_field, dev), torch.linspace(0, 1, steps=nt),
                                    torch.linspace(0, 1, steps=nh), torch.linspace(0, 1, steps=nw),
                                    "catmull_rom")
        return lat.to(out_dev)


# ------------------------------------------------------------------ estimators


def estimate_global_motion(image, pixel_spacing, reference_frame=None, b_factor=500,
                           frequency_range=(300, 10), device=None):
    """Whole-frame cross-correlation shift estimate (estimate_motion_xc.py:21-135).
    Returns the (2,t,1,1) float32 deformation field in Angstrom (integer px shifts x
    pixel_spacing; the reference frame's entry is exactly 0)."""
    with gpu_entry(image, device) as (out_dev, dev):
        img = _stage(image, dev, keep_half=True)  # fp16 stacks: K1 reads the 16-bit samples (4096-column frames)
        t = img.shape[0]
        ref = t // 2 if reference_frame is None else reference_frame
        normalize_frame_index(ref, t)  # IndexError outside [-t, t), as filtered_fft[ref] (xc.py:101)
        say(f"Cross-correlation whole image: using frame {ref} as reference")
        shifts = engine.global_shifts(img, ref, float(pixel_spacing), float(b_factor), frequency_range)
        if VERBOSE:
            say(f"Estimated shifts range: y=[{shifts[:, 0].min():.1f}, {shifts[:, 0].max():.1f}], "
                f"x=[{shifts[:, 1].min():.1f}, {shifts[:, 1].max():.1f}]")
        return image_shifts_to_deformation_field(shifts, pixel_spacing).to(out_dev)


def _check_refine_call(t, reference_frame, max_iterations, convergence_threshold):
    """The refinement's own argument rules, before any device is touched -> (reference frame, iterations, threshold)."""
    n_iter, thr = engine.check_refine_args(max_iterations, convergence_threshold)
    ref = t // 2 if reference_frame is None else reference_frame
    normalize_frame_index(ref, t)  # IndexError outside [-t, t)
    if t > engine.REFINE_MAX_FRAMES:
        raise NotImplementedError(f"{t} frames: the refinement takes at most {engine.REFINE_MAX_FRAMES}")
    return ref, n_iter, thr


def refine_global_motion(image, pixel_spacing, deformation_field=None, reference_frame=None, b_factor=500,
                         frequency_range=(300, 10), max_iterations=10, convergence_threshold=0.01,
                         return_history=False, device=None):
    """Iterative sub-pixel whole-frame alignment (the unblur / MotionCor2 scheme; the reference's example calls such a
    ``refine_alignment`` that the package never shipped, examples/ttMotion.py:264-285): every frame is aligned, to
    sub-pixel precision, against the sum of the OTHER aligned frames, until the shifts stop moving.  `image`: an fp32
    or fp16 (t, h, w) stack.  Returns the (2,t,1,1) float32 field in Angstrom, as ``estimate_global_motion`` does;
    the reference frame's entry is exactly 0.

    Start: ``estimate_global_motion``'s integer shifts, or a caller's rigid (2,t,1,1) `deformation_field` (Angstrom).
    Per iteration, on the masked, filtered spectra of ``estimate_global_motion`` (transformed once, no frame is read
    again): each frame's spectrum gets the phase ramp ``correct_motion_fast`` applies for the current shifts, is
    correlated with the mean of the others, and the residual -- the first maximum with the wrap-around rule plus the
    parabola offsets of the patch estimator's sub-pixel step, the three samples per axis taken circularly -- is added
    with the factor (t-1)/t (the frame's error against the mean of the others overstates it by t/(t-1)); then the
    reference frame's shift is subtracted from all.  The loop stops after the iteration whose largest residual is
    below `convergence_threshold` pixels (0: never), at the latest after `max_iterations`.  ``return_history=True``
    also returns the per-iteration largest residual as a CPU float tensor.  One frame returns zeros.

    `reference_frame` follows Python indexing (None: t // 2; outside [-t, t): IndexError).  Argument errors are
    raised before any device is touched.  At most 512 frames."""
    if not isinstance(image, torch.Tensor) or image.dim() != 3:
        raise ValueError(f"image must be (t, h, w), got {tuple(getattr(image, 'shape', ()))}")
    t = image.shape[0]
    ref, n_iter, thr = _check_refine_call(t, reference_frame, max_iterations=max_iterations,
                                          convergence_threshold=convergence_threshold)
    if deformation_field is not None:
        _check_fast_field(deformation_field, t)
    want_history = bool(return_history)
    with gpu_entry(image, device) as (out_dev, dev):
        img = _stage(image, dev, keep_half=True)
        ps = float(pixel_spacing)
        shifts, hist = engine.global_shifts_refined(img, ref, ps, float(b_factor), tuple(frequency_range),
                                                    _start_shifts(deformation_field, ps, dev), n_iter, thr)
        field = image_shifts_to_deformation_field(shifts, pixel_spacing).to(out_dev)
        return (field, hist) if want_history else field


def _start_shifts(deformation_field, ps, dev):
    """(t, 2) px start shifts of the refinement from a rigid (2,t,1,1) Angstrom field, or None."""
    if deformation_field is None:
        return None
    return (deformation_field.detach().to(device=dev, dtype=torch.float32)[:, :, 0, 0].transpose(0, 1) / ps).contiguous()


def refine_global_motion_raw(movie, gain, pixel_spacing, deformation_field=None, reference_frame=None, b_factor=500,
                             frequency_range=(300, 10), mean_zero=True, hot_pixel_threshold=None, max_iterations=10,
                             convergence_threshold=0.01, return_history=False, device=None):
    """``refine_global_motion(condition_movie(movie, gain, mean_zero, hot_pixel_threshold), ...)`` for a RAW uint8 /
    int16 movie without the conditioned fp32 movie: the spectra are those ``motion_correct_raw`` and
    ``motion_correct_raw_fast`` estimate on (the row transform reads the raw bytes, hot pixels enter as sparse
    corrections, engine.RawMovie), and the iterations only touch those spectra.  Returns the (2,t,1,1) Angstrom
    field (and the history); feed it to ``motion_correct_sum_fast_raw`` or ``motion_correct_sum_raw`` for the sums,
    again without an fp32 movie.  fp16 / fp32 movies, shapes without the fused kernels and a hot-pixel list overflow
    take exactly condition_movie followed by refine_global_motion."""
    thr_hot = engine.check_hot_pixel_threshold(hot_pixel_threshold)  # every argument rule before any device
    _check_raw_args(movie, gain)
    t = movie.shape[0]
    ref, n_iter, thr = _check_refine_call(t, reference_frame, max_iterations=max_iterations,
                                          convergence_threshold=convergence_threshold)
    if deformation_field is not None:
        _check_fast_field(deformation_field, t)
    want_history = bool(return_history)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, gd = _stage_raw(movie, gain, dev)
        ps = float(pixel_spacing)
        args = (ref, ps, float(b_factor), tuple(frequency_range), _start_shifts(deformation_field, ps, dev), n_iter,
                thr)
        res, _ = _raw_or_conditioned(raw, gd, mean_zero, thr=thr_hot,
                                     fused=lambda rm: engine.global_shifts_raw_refined(rm, *args),
                                     conditioned=lambda img: engine.global_shifts_refined(img, *args))
        field = image_shifts_to_deformation_field(res[0], pixel_spacing).to(out_dev)
        return (field, res[1]) if want_history else field


def _check_local_refine_call(movie, patch_sidelength, deformation_field, reference_frame, max_iterations,
                             convergence_threshold, what):
    """Argument rules of the patch refinement, before any device is touched -> (patch side, reference frame,
    iterations, threshold)."""
    if not isinstance(movie, torch.Tensor) or movie.dim() != 3:
        raise ValueError(f"{what} must be (t, h, w), got {tuple(getattr(movie, 'shape', ()))}")
    t, h, w = movie.shape
    ref, n_iter, thr = _check_refine_call(t, reference_frame, max_iterations=max_iterations,
                                          convergence_threshold=convergence_threshold)
    p = _check_patch_sidelength(patch_sidelength, (h, w))
    if deformation_field is not None:
        _check_field_4d(deformation_field, "deformation_field must be a (2, nt, gh, gw) tensor")
    return p, ref, n_iter, thr


def _local_refine_result(res, ps, want_history, out_dev):
    shifts, hist, centres = res
    field = (shifts.permute(3, 0, 1, 2) * ps).contiguous().to(out_dev)
    return (field, centres.to(out_dev), hist) if want_history else (field, centres.to(out_dev))


def refine_local_motion(image, pixel_spacing, patch_sidelength=1024, deformation_field=None, reference_frame=None,
                        b_factor=500, frequency_range=(300, 10), max_iterations=10, convergence_threshold=0.01,
                        return_history=False, device=None):
    """Iterative sub-pixel patch alignment (local motion; MotionCor2's scheme, and what the reference's example does
    with five passes of the patch estimator, examples/ttMotion.py:287-329): every patch of every frame is aligned, to
    sub-pixel precision, against the mean of the same patch of the OTHER aligned frames, until the shifts stop
    moving.  `image`: an fp32 or fp16 (t, h, w) stack (fp16 is read as it is by the 1024-px patch kernel and widened
    once otherwise).  Returns ``(field (2, t, gh, gw) float32 in Angstrom, centres (t, gh, gw, 3) int64[, history])``
    on the lattice ``estimate_motion_cross_correlation_patches`` uses.  The field's global mean is NOT subtracted:
    frame `reference_frame` is the coordinate system and its field is exactly 0 in every patch, as in
    ``refine_global_motion``.  No outlier rejection, no temporal smoothing.

    Start: `deformation_field` (Angstrom; (2, t, 1, 1) from ``refine_global_motion`` or any (2, nt, gh', gw')), divided
    by the pixel spacing and resampled to (t, gh, gw) as ``resample_deformation_field`` does; None: the result of
    ``refine_global_motion`` on the same stack with the same `b_factor`, `frequency_range` and `reference_frame` at
    its default iteration settings.  Every job's window is cut ONCE, at the patch origin + o with o = the start
    rounded to whole pixels (halves to even) and clamped per axis so that the window stays inside the frame; the
    offset needs no coarser unit for any storage type.  The windows are normalised with the central-box statistics
    of the stack as it is, masked once and transformed once.  Per iteration, on those spectra only (no frame is read
    again and no warped movie is written): the phase ramp for s - o, the leave-one-out mean per patch, the residual
    -- first maximum with the wrap-around rule plus the parabola offsets of the patch estimator's sub-pixel step, the
    three samples per axis taken circularly -- added with the factor (t-1)/t, then the reference frame's shift is
    subtracted per patch.  The loop stops after the iteration whose largest residual over all frames and patches is
    below `convergence_threshold` pixels (0: never, and nothing is read back inside the loop), at the latest after
    `max_iterations`.  ``return_history=True`` appends the per-iteration largest residual as a CPU float tensor.
    One frame returns zeros.

    `reference_frame` follows Python indexing (None: t // 2; outside [-t, t): IndexError).  Argument errors are raised
    before any device is touched.  At most 512 frames."""
    p, ref, n_iter, thr = _check_local_refine_call(
        image, patch_sidelength, deformation_field, reference_frame=reference_frame, max_iterations=max_iterations,
        convergence_threshold=convergence_threshold, what="image")
    want_history = bool(return_history)
    with gpu_entry(image, device) as (out_dev, dev):
        img = _stage(image, dev, keep_half=True)
        ps = float(pixel_spacing)
        field = None if deformation_field is None else _stage(deformation_field, dev)
        res = engine.local_shifts_refined(img, ps, p, field, ref, float(b_factor), tuple(frequency_range), n_iter, thr)
        return _local_refine_result(res, ps, want_history=want_history, out_dev=out_dev)


def refine_local_motion_raw(movie, gain, pixel_spacing, patch_sidelength=1024, deformation_field=None,
                            reference_frame=None, b_factor=500, frequency_range=(300, 10), max_iterations=10,
                            convergence_threshold=0.01, return_history=False, device=None, mean_zero=True,
                            hot_pixel_threshold=None):
    """``refine_local_motion(condition_movie(movie, gain, mean_zero, hot_pixel_threshold), ...)`` for a RAW uint8 /
    int16 movie without the conditioned fp32 movie: the default start comes from ``refine_global_motion_raw``'s
    route, the patch row pass reads the raw bytes and forms ``raw * gain - frame mean`` on the fly
    (engine.RawMovie), and the iterations only touch the patch spectra.  Returns ``(field, centres[, history])``.
    The sums of the example's pipeline follow, still without an fp32 movie, from
    ``motion_correct_sum_raw(movie, gain, field, pixel_spacing, dose_per_frame=..., return_plain_sum=True)``.

    Fused route: u8 / i16 movies, 1024-px patches, no `hot_pixel_threshold`, frame shapes the raw kernels take.
    Every other case runs exactly condition_movie followed by refine_local_motion."""
    thr_hot = engine.check_hot_pixel_threshold(hot_pixel_threshold)  # every argument rule before any device
    _check_raw_args(movie, gain)
    p, ref, n_iter, thr = _check_local_refine_call(
        movie, patch_sidelength, deformation_field, reference_frame=reference_frame, max_iterations=max_iterations,
        convergence_threshold=convergence_threshold, what="movie")
    want_history = bool(return_history)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, gd = _stage_raw(movie, gain, dev)
        ps = float(pixel_spacing)
        field = None if deformation_field is None else _stage(deformation_field, dev)
        args = (ps, p, field, ref, float(b_factor), tuple(frequency_range), n_iter, thr)
        # (the engine refuses a hot-pixel threshold)
        res, _ = _raw_or_conditioned(raw, gd, mean_zero, thr=thr_hot,
                                     fused=lambda rm: engine.local_shifts_raw_refined(rm, *args),
                                     conditioned=lambda img: engine.local_shifts_refined(img, *args),
                                     allow_fused=thr_hot is None)
        return _local_refine_result(res, ps, want_history=want_history, out_dev=out_dev)


def _check_patch_estimate_args(t, reference_frame, reference_strategy, sub_pixel_refinement, outlier_rejection):
    """The patch estimator's own argument rules -> the reference frame it uses."""
    if reference_strategy not in ("middle_frame", "mean_except_current"):
        raise ValueError(f"Unknown reference_strategy: {reference_strategy}")
    ref = t // 2 if reference_frame is None else reference_frame
    if reference_strategy == "middle_frame":
        normalize_frame_index(ref, t)  # lazy_patch_grid[ref] (xc.py:306): IndexError outside [-t, t)
    else:
        ref = t // 2  # mean_except_current never reads reference_frame (xc.py:310-328)
    if BUG_COMPATIBLE and outlier_rejection and not sub_pixel_refinement:
        # Q12: integer peak coordinates reach torch.std at estimate_motion_xc.py:577
        raise RuntimeError("std and var only support floating point and complex dtypes")
    return ref


def estimate_motion_cross_correlation_patches(
    image, pixel_spacing, reference_frame=None, reference_strategy="mean_except_current",
    b_factor=500, frequency_range=(300, 10), patch_sidelength=1024, sub_pixel_refinement=True,
    temporal_smoothing=True, smoothing_window_size=5, deformation_field=None,
    outlier_rejection=True, outlier_threshold=3.0, device=None,
):
    """Per-patch cross-correlation shift estimate (estimate_motion_xc.py:138-411).
    Returns ((2,t,gh,gw) Angstrom field with its global mean subtracted,
    (t,gh,gw,3) int64 patch centres)."""
    with gpu_entry(image, device) as (out_dev, dev):
        # an fp16 stack stays fp16 unless a prior field has to be applied first (that path normalises
        # and resamples in fp32)
        img = _stage(image, dev, keep_half=deformation_field is None)
        t, h, w = img.shape
        ref = _check_patch_estimate_args(t, reference_frame, reference_strategy,
                                         sub_pixel_refinement=sub_pixel_refinement,
                                         outlier_rejection=outlier_rejection)
        stats = engine.central_box_stats(img)  # statistics of the *uncorrected* stack (Q9)
        field0 = None
        if deformation_field is not None:
            if deformation_field.device != out_dev:
                deformation_field = deformation_field.clone()  # the reference's .to(device) copy
            norm = engine.normalize(img, stats)
            stats = None
            if tuple(deformation_field.shape[-2:]) == (1, 1):
                say("Applying single patch deformation field using correct_motion_fast")
                img = _correct_motion_fast_impl(norm, deformation_field, dev, mutate=BUG_COMPATIBLE)
            else:
                say("Applying full deformation field using correct_motion")
                lat = engine.frame_lattices(_stage(deformation_field, dev), t, "bspline")
                img, _ = engine.warp(norm, lat, float(pixel_spacing))
            # the prior field (after Q1's in-place negation, if any) is the accumulator base
            from .lattice import patch_grid_centers

            cy, cx = patch_grid_centers(t, h, w, int(patch_sidelength))
            field0 = resample_deformation_field(_stage(deformation_field, dev), (t, len(cy), len(cx)))
        field, centers = engine.patch_field(
            img, stats, float(pixel_spacing), ref, reference_strategy, float(b_factor), frequency_range,
            patch_sidelength, bool(sub_pixel_refinement), bool(temporal_smoothing),
            int(smoothing_window_size), field0, bool(outlier_rejection), float(outlier_threshold))
        return field.to(out_dev), centers.to(out_dev)


def estimate_motion(image, pixel_spacing, patch_sidelength=None, **kwargs):
    """Convenience alias (ours, not the reference's): global estimate when
    ``patch_sidelength`` is None, else the patch estimate (field only)."""
    if patch_sidelength is None:
        return estimate_global_motion(image, pixel_spacing, **kwargs)
    return estimate_motion_cross_correlation_patches(
        image, pixel_spacing, patch_sidelength=patch_sidelength, **kwargs)[0]


# ------------------------------------------------------------------ correctors


def correct_motion(image, deformation_grid, pixel_spacing, grad=False, grid_type="catmull_rom",
                   device=None):
    """Apply a (2,nt,gh,gw) Angstrom deformation field (correct_motion.py:18-78).
    Returns the (t,h,w) corrected frames, detached.  ``grad=True`` (autograd through
    the resampling) is not available on the HIP path."""
    with gpu_entry(image, device) as (out_dev, dev):
        if grad:
            raise NotImplementedError("grad=True is not supported by the HIP path (forward only)")
        img = _stage(image, dev, keep_half=True)
        lat = engine.frame_lattices(_stage(deformation_grid, dev), img.shape[0], grid_type)
        frames, _ = engine.warp(img, lat, float(pixel_spacing), want_frames=True, want_sum=False,
                                rigid=RIGID_FAST_PATH and _is_rigid(deformation_grid))
        return frames.to(out_dev)


def _grid_data_and_type(grid, default="catmull_rom"):
    """A (c,nt,nh,nw) tensor, or a spline-grid object of the reference's dependency
    (torch_cubic_spline_grids: `.data` holds the control points, the class name the basis)."""
    if isinstance(grid, torch.Tensor):
        return grid, default
    data = getattr(grid, "data", None)
    if not isinstance(data, torch.Tensor):
        raise TypeError("expected a (2, nt, nh, nw) tensor or a cubic spline grid object with a .data tensor")
    return data, ("bspline" if "bspline" in type(grid).__name__.lower() else "catmull_rom")


def _wants_grad(grid) -> bool:
    if isinstance(grid, torch.Tensor):
        return grid.requires_grad
    params = getattr(grid, "parameters", None)
    return any(p.requires_grad for p in params()) if callable(params) else False


def correct_motion_two_grids(image, new_deformation_grid, base_deformation_grid, pixel_spacing, grad=True,
                             device=None):
    """correct_motion.py:188-299 -- the frames resampled through the SUM of two spline grids
    (an optimisable one and a frozen base), each evaluated on the (10 gh, 10 gw) lattice of the
    new grid.  The grids are (2,nt,nh,nw) tensors (Catmull-Rom) or grid objects of the reference's
    spline package; they may differ in resolution and basis.  Forward only: with ``grad=True`` (the
    reference's default) and a grid that requires gradients the result is attached to that grid, as
    in the reference, but calling ``backward`` through it raises NotImplementedError."""
    with gpu_entry(image, device) as (out_dev, dev):
        img = _stage(image, dev)
        new, new_type = _grid_data_and_type(new_deformation_grid)
        base, base_type = _grid_data_and_type(base_deformation_grid)
        t = img.shape[0]
        _, _, gh, gw = new.shape
        lin = lambda n: torch.linspace(0, 1, steps=n)
        lat = (engine.spline_lattice(_stage(new, dev), lin(t), lin(10 * gh), lin(10 * gw), new_type)
               + engine.spline_lattice(_stage(base, dev), lin(t), lin(10 * gh), lin(10 * gw), base_type))
        frames, _ = engine.warp(img, lat.permute(1, 0, 2, 3).contiguous(), float(pixel_spacing),
                                want_frames=True, want_sum=False)
        frames = frames.to(out_dev)
        if grad and _wants_grad(new_deformation_grid):
            # the reference returns frames attached to the new grid's graph; the forward here is the
            # same, the backward is refused where it would be needed
            params = ([new_deformation_grid] if isinstance(new_deformation_grid, torch.Tensor)
                      else [p for p in new_deformation_grid.parameters() if p.requires_grad])
            frames = _ForwardOnly.apply(frames, *params)
        return frames


class _ForwardOnly(torch.autograd.Function):
    """Marks a HIP result as depending on `params`; differentiating through it fails loudly."""

    @staticmethod
    def forward(ctx, frames, *params):
        return frames.view_as(frames)

    @staticmethod
    def backward(ctx, gout):
        raise NotImplementedError("gradients through the HIP resampling kernels are not available "
                                  "(forward only); use grad=False")


def correct_motion_slow(image, deformation_grid, grad=False, device=None):
    """correct_motion.py:302-427 -- the (2,nt,nh,nw) field evaluated (Catmull-Rom) at EVERY pixel
    (t_i, y/(h-1), x/(w-1)) and used as PIXEL shifts (no pixel spacing), then bicubic resampling.
    One frame at a time: the per-pixel shifts are a tensor-product spline lattice of the frame's
    own size, which the general warp kernel consumes directly (its bicubic lattice upsample is the
    identity at the lattice nodes up to 1e-4 of the shift difference between adjacent pixels)."""
    with gpu_entry(image, device) as (out_dev, dev):
        if grad:
            raise NotImplementedError("grad=True is not supported by the HIP path (forward only)")
        img = _stage(image, dev)
        field = _stage(deformation_grid, dev)
        t, h, w = img.shape
        times = torch.linspace(0, 1, steps=t)
        uy = torch.arange(h, dtype=torch.float32) / float(h - 1)
        ux = torch.arange(w, dtype=torch.float32) / float(w - 1)
        out = torch.empty_like(img)
        for f in range(t):
            lat = engine.spline_lattice(field, times[f:f + 1], uy, ux, "catmull_rom")  # (2, 1, h, w)
            frames, _ = engine.warp(img[f:f + 1], lat.permute(1, 0, 2, 3).contiguous(), 1.0,
                                    want_frames=True, want_sum=False)
            out[f] = frames[0]
        return out.to(out_dev)


def motion_correct_sum(image, deformation_grid, pixel_spacing, grid_type="catmull_rom", device=None,
                       return_frames=False, dose_per_frame=None, pre_exposure=0.0, voltage=300.0):
    """Fused correct_motion + the caller-side ``torch.sum(movie, dim=0)`` of the
    reference's pipeline (examples/ttMotion.py:398): returns the (h,w) aligned sum
    (and the frames when asked) without a second pass over the stack.  With
    ``dose_per_frame`` (e/A^2) the sum is exposure-filtered as in the reference's
    ``dose_weight`` step (examples/ttMotion.py:331-351; see ``dose_weighted_sum``)."""
    with gpu_entry(image, device) as (out_dev, dev):
        img = _stage(image, dev, keep_half=True)
        lat = engine.frame_lattices(_stage(deformation_grid, dev), img.shape[0], grid_type)
        rigid = RIGID_FAST_PATH and _is_rigid(deformation_grid)
        total, _, frames = engine.corrected_sums(img, lat, pixel_spacing, rigid, dose_per_frame, pre_exposure,
                                                 voltage, False, return_frames)
        return (total.to(out_dev), frames.to(out_dev)) if return_frames else total.to(out_dev)


def condition_movie(movie, gain=None, mean_zero=True, device=None, hot_pixel_threshold=None,
                    return_hot_counts=False):
    """Raw detector frames -> the fp32 stack the estimators expect: ``movie * gain`` (a (h,w)
    multiplicative gain reference, already flipped / rotated as needed) and, per frame,
    minus its own mean -- the ``gain_correct`` and ``set_frames_mean_zero`` steps of the
    reference's pipeline (examples/ttMotion.py:90-121, 174-199) done on the device straight
    from uint8 / int16 / float16 / float32 storage.  `hot_pixel_threshold` (the example's
    ``remove_hot_pixels`` uses 10.0; None = off) adds that step between the two: a pixel more than
    `threshold` standard deviations from its frame's mean is hot -- the example's detection -- and
    is replaced by the mean of its neighbours that are not hot (the example draws a RANDOM
    neighbour: that part has no deterministic counterpart and the rule here is ours).
    `return_hot_counts`: also the (t,) int32 number of hot pixels found per frame."""
    with gpu_entry(movie, device) as (out_dev, dev):
        res = engine.condition_movie(movie.detach().to(dev), gain, bool(mean_zero), hot_pixel_threshold,
                                     bool(return_hot_counts))
        if return_hot_counts:
            return res[0].to(out_dev), res[1].to(out_dev)
        return res.to(out_dev)


def _check_dose(dose_per_frame):
    """None, or a finite dose >= 0 (e/A^2 per frame) as a float; ValueError otherwise (before any device is touched)."""
    if dose_per_frame is None:
        return None
    try:
        v = float(dose_per_frame)
    except (TypeError, ValueError):
        raise ValueError(f"dose_per_frame must be a finite number >= 0, got {dose_per_frame!r}") from None
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError(f"dose_per_frame must be a finite number >= 0, got {dose_per_frame!r}")
    return v


def motion_correct_raw(movie, gain, pixel_spacing, reference_frame=None, b_factor=500, frequency_range=(300, 10),
                       grid_type="catmull_rom", mean_zero=True, return_frames=False, device=None,
                       hot_pixel_threshold=None, return_hot_counts=False, dose_per_frame=None, pre_exposure=0.0,
                       voltage=300.0):
    """The reference pipeline's gain_correct -> set_frames_mean_zero -> estimate_global_motion -> correct_motion
    -> sum (examples/ttMotion.py:90-121, 180-199, 286-398) for a RAW uint8 / int16 movie, with the conditioning
    fused into the kernels that read the raw bytes: one statistics pass, then the estimator's row transform and
    the rigid warp compute ``raw * gain - frame mean`` on the fly.  No conditioned fp32 movie is allocated.
    Returns ``(field (2,t,1,1) Angstrom, sum (h,w)[, frames (t,h,w)][, hot counts (t,) int32])`` -- what
    ``condition_movie`` followed by ``estimate_global_motion`` and ``motion_correct_sum`` return.  Fused kernels
    exist for power-of-two frame widths and the K3 formats (5760 / 11520 columns), rows of whole quads, at most
    256 frames; any other shape takes exactly that route, on an fp32 copy.

    ``hot_pixel_threshold`` (the example uses 10.0) adds the example's remove_hot_pixels step
    (examples/ttMotion.py:127-172) between the gain and the mean, with condition_movie's deterministic
    replacement; the fused route applies the few hot pixels as sparse corrections (engine.RawMovie).  A threshold
    that finds more hot pixels than the fused list holds takes the condition_movie route.  ``return_hot_counts``
    appends the number of hot pixels per frame (zeros without a threshold).

    ``dose_per_frame`` (e/A^2; with ``pre_exposure`` and ``voltage``) makes the returned sum the exposure-filtered
    one, as ``motion_correct_sum(..., dose_per_frame=...)`` computes it: on the row-major frame sizes the frames are
    warped from the raw bytes, transformed and weighted a chunk at a time (engine.warp_dose_weighted_sum_raw); the
    field is the same.  For the plain sum as well, pass the field to ``motion_correct_sum_raw(...,
    return_plain_sum=True)``."""
    thr = engine.check_hot_pixel_threshold(hot_pixel_threshold)  # ValueError before any device is touched
    dose = _check_dose(dose_per_frame)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, gd = _stage_raw(movie, gain, dev)
        t = raw.shape[0]
        ref = t // 2 if reference_frame is None else int(reference_frame)
        ps = float(pixel_spacing)

        def route(estimate):  # the same steps on a RawMovie and on the conditioned movie
            def run(src):
                shifts = estimate(src, ref, ps, float(b_factor), tuple(frequency_range))
                field = image_shifts_to_deformation_field(shifts, ps)
                lat = engine.frame_lattices(field.contiguous(), t, grid_type)
                total, _, frames = engine.corrected_sums(src, lat, ps, True, dose, pre_exposure, voltage, False,
                                                         bool(return_frames))
                return field, total, frames
            return run

        (field, total, frames), counts = _raw_or_conditioned(raw, gd, mean_zero, thr=thr,
                                                             fused=route(engine.global_shifts_raw),
                                                             conditioned=route(engine.global_shifts))
        out = [field.to(out_dev), total.to(out_dev)]
        if return_frames:
            out.append(frames.to(out_dev))
        if return_hot_counts:
            out.append(_hot_counts_out(counts, t, out_dev))
        return tuple(out)


def motion_correct_raw_patches(movie, gain, pixel_spacing, patch_sidelength=1024, reference_frame=None,
                               reference_strategy="mean_except_current", b_factor=500, frequency_range=(300, 10),
                               sub_pixel_refinement=True, temporal_smoothing=True, smoothing_window_size=5,
                               deformation_field=None, outlier_rejection=True, outlier_threshold=3.0,
                               grid_type="catmull_rom", mean_zero=True, return_frames=False, device=None,
                               hot_pixel_threshold=None, return_hot_counts=False):
    """The local-motion flow of the reference pipeline for a RAW uint8 / int16 movie: ``condition_movie(movie, gain,
    mean_zero, hot_pixel_threshold)`` then ``estimate_motion_cross_correlation_patches`` and ``motion_correct_sum``
    with the field it returns.  Returns ``(field (2,t,gh,gw) Angstrom, centres (t,gh,gw,3) int64, sum (h,w)[, frames
    (t,h,w)][, hot counts (t,) int32])``.  The exposure-filtered sum (the example's ``dose_weight`` step) of the same
    movie comes from ``motion_correct_sum_raw(movie, gain, field, pixel_spacing, grid_type=grid_type,
    dose_per_frame=..., return_plain_sum=True)`` with the field returned here: again no fp32 movie.

    Fused route (no conditioned fp32 movie is allocated): u8 / i16 movies, 1024-px patches, no prior
    ``deformation_field`` and no ``hot_pixel_threshold``.  The patch row pass and the field warp read the raw bytes
    and form ``raw * gain - frame mean`` on the fly (engine.patch_field_raw, engine.warp_field_raw); the results
    differ from the conditioned route only by the fp32 rounding of that conditioning.  Every other case, and any
    shape the raw kernels do not take, runs exactly the conditioned route."""
    if reference_strategy not in ("middle_frame", "mean_except_current"):
        raise ValueError(f"Unknown reference_strategy: {reference_strategy}")
    thr = engine.check_hot_pixel_threshold(hot_pixel_threshold)  # ValueError before any device is touched
    p = _check_patch_sidelength(patch_sidelength)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, gd = _stage_raw(movie, gain, dev)
        t = raw.shape[0]
        ps = float(pixel_spacing)
        allow_fused = deformation_field is None and thr is None
        ref = None
        if allow_fused and raw.dtype in RAW_DTYPES:  # the estimator's own argument rules, before any launch
            ref = _check_patch_estimate_args(t, reference_frame, reference_strategy,
                                             sub_pixel_refinement=sub_pixel_refinement,
                                             outlier_rejection=outlier_rejection)

        def fused(rm):
            field, centers = engine.patch_field_raw(
                rm, ps, ref, reference_strategy, float(b_factor), frequency_range, p,
                bool(sub_pixel_refinement), bool(temporal_smoothing), int(smoothing_window_size),
                bool(outlier_rejection), float(outlier_threshold))
            lat = engine.frame_lattices(field, t, grid_type)
            # (a single patch: motion_correct_sum's rigid warp)
            total, _, frames = engine.corrected_sums(rm, lat, ps, RIGID_FAST_PATH and _is_rigid(field),
                                                     want_frames=bool(return_frames))
            return field, centers, total, frames

        def conditioned(img):
            field, centers = estimate_motion_cross_correlation_patches(
                img, ps, reference_frame=reference_frame, reference_strategy=reference_strategy, b_factor=b_factor,
                frequency_range=frequency_range, patch_sidelength=p,
                sub_pixel_refinement=sub_pixel_refinement, temporal_smoothing=temporal_smoothing,
                smoothing_window_size=smoothing_window_size, deformation_field=deformation_field,
                outlier_rejection=outlier_rejection, outlier_threshold=outlier_threshold)
            res = motion_correct_sum(img, field, ps, grid_type=grid_type, return_frames=bool(return_frames))
            return (field, centers, *(res if return_frames else (res, None)))

        (field, centers, total, frames), counts = _raw_or_conditioned(
            raw, gd, mean_zero, thr=thr, fused=fused, conditioned=conditioned, allow_fused=allow_fused)
        out = [field.to(out_dev), centers.to(out_dev), total.to(out_dev)]
        if return_frames:
            out.append(frames.to(out_dev))
        if return_hot_counts:
            out.append(_hot_counts_out(counts, t, out_dev))
        return tuple(out)


def motion_correct_sum_raw(movie, gain, deformation_grid, pixel_spacing, grid_type="catmull_rom", mean_zero=True,
                           hot_pixel_threshold=None, dose_per_frame=None, pre_exposure=0.0, voltage=300.0,
                           return_plain_sum=False, return_frames=False, device=None):
    """``motion_correct_sum`` of ``condition_movie(movie, gain, mean_zero, hot_pixel_threshold)`` for a RAW uint8 /
    int16 movie and a (2,t,gh,gw) Angstrom field -- from ``motion_correct_raw``, ``motion_correct_raw_patches`` or
    ``read_deformation_field_from_csv`` -- without the conditioned fp32 movie: the warps read the raw bytes and form
    ``raw * gain - frame mean`` on the fly.  Without ``dose_per_frame`` the result is the plain aligned sum, bit for
    bit the one motion_correct_raw / motion_correct_raw_patches return for that field.  With it (e/A^2; with
    ``pre_exposure`` and ``voltage``) the sum is exposure-filtered as the example's ``dose_weight`` step
    (examples/ttMotion.py:331-351, 398-404) and motion_correct_sum(..., dose_per_frame=...): on the row-major frame
    sizes the frames are warped, transformed and weighted a chunk at a time, so the corrected movie is not held
    either.  ``return_plain_sum`` (needs a dose) also returns the plain sum, accumulated by the same warp launches:
    the example's two images for one pass over the movie.

    Returns ``sum (h,w)``, or the tuple ``(sum[, plain sum][, frames (t,h,w)])``.  A (2,t,1,1) field takes the rigid
    warp.  fp16 / fp32 movies, shapes without fused kernels, a local field with ``hot_pixel_threshold`` (the local
    raw warp has no hot-pixel corrections) and a hot-pixel list overflow take exactly the conditioned route."""
    dose = _check_fast_sum_args(dose_per_frame, return_plain_sum)  # every argument rule before any device is touched
    thr = engine.check_hot_pixel_threshold(hot_pixel_threshold)
    _check_field_4d(deformation_grid, "deformation_grid must be a (2, nt, gh, gw) tensor")
    _check_raw_args(movie, gain)
    want_plain, want_frames = bool(return_plain_sum), bool(return_frames)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, gd = _stage_raw(movie, gain, dev)
        t = raw.shape[0]
        ps = float(pixel_spacing)
        field = _stage(deformation_grid, dev)
        rigid = RIGID_FAST_PATH and _is_rigid(field)

        def fused(rm):
            lat = engine.frame_lattices(field, t, grid_type)
            return engine.corrected_sums(rm, lat, ps, rigid, dose, pre_exposure, voltage, want_plain, want_frames)

        def conditioned(img):  # motion_correct_sum, once more without the dose for the plain sum
            res = motion_correct_sum(img, field, ps, grid_type=grid_type, return_frames=want_frames,
                                     dose_per_frame=dose, pre_exposure=pre_exposure, voltage=voltage)
            total, frames = res if want_frames else (res, None)
            return total, (motion_correct_sum(img, field, ps, grid_type=grid_type) if want_plain else None), frames

        (total, plain, frames), _ = _raw_or_conditioned(raw, gd, mean_zero, thr=thr, fused=fused,
                                                        conditioned=conditioned)
        out = [total.to(out_dev)]
        if want_plain:
            out.append(plain.to(out_dev))
        if want_frames:
            out.append(frames.to(out_dev))
        return out[0] if len(out) == 1 else tuple(out)


def dose_weighted_sum(movie, pixel_spacing, dose_per_frame, pre_exposure=0.0, voltage=300.0, device=None):
    """``sum_f irfft2(q_f * rfft2(frame_f))`` with the Grant & Grigorieff exposure filter
    ``q_f = exp(-0.5 N_f / N_c(|k|))`` normalised by ``sqrt(sum_f q_f^2)``: the reference
    pipeline's ``dose_weight(movie)`` (examples/ttMotion.py:331-351: rfft2(norm='ortho') ->
    torch_fourier_filter dose_weight_movie(crit_exposure_bfactor=-1) -> irfft2 -> sum).  The
    third-party filter is not part of the reference tree and untested there: parity unpinned."""
    with gpu_entry(movie, device) as (out_dev, dev):
        return engine.dose_weighted_sum(_stage(movie, dev), float(pixel_spacing), float(dose_per_frame),
                                        float(pre_exposure), float(voltage)).to(out_dev)


def estimate_local_motion(image, pixel_spacing, patch_shape, deformation_field_resolution,
                          initial_deformation_field=None, device=None, n_iterations=100, b_factor=500,
                          frequency_range=(300, 10), optimizer_type="adam", grid_type="catmull_rom",
                          loss_type="mse", optimizer_kwargs=None, return_trajectory=False,
                          trajectory_kwargs=None):
    """Refine a (2, nt, nh, nw) spline deformation field by gradient descent on the agreement of
    Fourier-shifted patches with the mean of the other frames (estimate_motion_optimizer.py:28-439;
    same arguments, defaults, return values and error messages).  The loss and its analytic
    gradient are HIP kernels over patch spectra that are transformed once (local_motion.py)."""
    # CPU tensors are staged to the GPU and the field comes back on `out_dev`
    with gpu_entry(image, device) as (out_dev, dev):
        from . import local_motion
        from .optimization_state import OptimizationTracker

        img = _stage(image, dev)
        if grid_type not in ("catmull_rom", "bspline"):
            raise ValueError(f"Invalid grid type: {grid_type}. Must be 'catmull_rom' or 'bspline'.")
        res = tuple(int(r) for r in deformation_field_resolution)
        trajectory = None
        if return_trajectory:
            tk = trajectory_kwargs if trajectory_kwargs is not None else {}
            tk.setdefault("sample_every_n_steps", 1)
            tk.setdefault("total_steps", n_iterations)
            trajectory = OptimizationTracker(**tk)
        if initial_deformation_field is None:
            init = torch.zeros((2, *res), dtype=torch.float32, device=dev)
        else:
            init = resample_deformation_field(_stage(initial_deformation_field.detach(), dev), res).contiguous()
            init = init - torch.mean(init)
        final = local_motion.estimate_local_motion(img, float(pixel_spacing), patch_shape, res, init, n_iterations,
                                                   b_factor, frequency_range, optimizer_type, grid_type, loss_type,
                                                   optimizer_kwargs, trajectory)
        final = final.to(out_dev)
        return (final, trajectory) if return_trajectory else final


def _correct_motion_fast_impl(img_dev, deformation_grid, dev, mutate):
    if tuple(deformation_grid.shape[-2:]) != (1, 1):
        raise ValueError(
            f"Expected single patch deformation field with shape (2, t, 1, 1), "
            f"but got shape {deformation_grid.shape}. "
            f"Final two dimensions must be (1, 1) for single patch correction."
        )
    shifts = -deformation_grid.detach()[:, :, 0, 0].transpose(0, 1).to(torch.float32)
    if mutate:
        deformation_grid.mul_(-1)  # Q1: correct_motion.py:473-474 negates the caller's tensor
    return engine.fourier_shift(img_dev, shifts.to(dev))


def correct_motion_fast(image, deformation_grid, device=None):
    """Rigid correction by a Fourier phase ramp (correct_motion.py:430-498); field
    values are used as pixels.  With BUG_COMPATIBLE the caller's `deformation_grid` is
    negated in place exactly when the reference would do so (grid already on the
    target device)."""
    with gpu_entry(image, device) as (out_dev, dev):
        mutate = BUG_COMPATIBLE and (device is None or deformation_grid.device == torch.device(device))
        out = _correct_motion_fast_impl(_stage(image, dev), deformation_grid, dev, mutate=mutate)
        return out.to(out_dev)


def _check_fast_field(deformation_grid, t):
    """A rigid (2, t, 1, 1) field for the Fourier-shift sums; ValueError otherwise (before any device is touched).  A
    field with more than one patch gets correct_motion_fast's own message."""
    field = deformation_grid
    _check_field_4d(field, "deformation_grid must be a (2, t, 1, 1) tensor")
    if tuple(field.shape[-2:]) != (1, 1):
        raise ValueError(
            f"Expected single patch deformation field with shape (2, t, 1, 1), "
            f"but got shape {field.shape}. "
            f"Final two dimensions must be (1, 1) for single patch correction."
        )
    if field.shape[1] != t:
        raise ValueError(f"deformation_grid has {field.shape[1]} time points, the movie {t} frames")


def _check_fast_sum_args(dose_per_frame, return_plain_sum):
    dose = _check_dose(dose_per_frame)
    if return_plain_sum and dose is None:
        raise ValueError("return_plain_sum needs dose_per_frame: without a dose the result is the plain sum")
    return dose


def _fast_sums(img, field, sums):
    """(dose-weighted sum or None, plain sum or None) of the fp32 stack `img` (on the device) shifted by the
    Angstrom `field` (on the device): the fused sums, or -- where they raise McorrUnsupported -- exactly
    correct_motion_fast(img, field / ps) followed by .sum(0) and dose_weighted_sum.  `sums`: engine.fast_shift_sums'
    trailing arguments (ps, dose, pre_exposure, voltage, want_plain)."""
    ps, dose, pre_exposure, voltage, want_plain = sums
    g = field / ps
    shifts = engine.fast_shifts(g)
    try:
        return engine.fast_shift_sums(img, shifts, ps, dose, pre_exposure, voltage, want_plain)
    except McorrUnsupported:
        cor = engine.fourier_shift(img, shifts)
        dw = None if dose is None else engine.dose_weighted_sum(cor, ps, dose, float(pre_exposure), float(voltage))
        plain = cor.sum(0) if (dose is None or want_plain) else None
        return dw, plain


def _fast_result(sums, want_plain, out_dev):
    dw, plain = sums
    if dw is None:
        return plain.to(out_dev)
    return (dw.to(out_dev), plain.to(out_dev)) if want_plain else dw.to(out_dev)


def motion_correct_sum_fast(image, deformation_grid, pixel_spacing, dose_per_frame=None, pre_exposure=0.0,
                            voltage=300.0, return_plain_sum=False, device=None):
    """The whole-image route of the example's pipeline after the estimate (examples/ttMotion.py:242-262, 390-404):
    ``correct_motion_fast`` (a Fourier phase ramp, no interpolation) followed by ``torch.sum`` and ``dose_weight``,
    without the shifted movie.  `image`: an fp32 or fp16 (t, h, w) stack; `deformation_grid`: a rigid (2, t, 1, 1)
    field in Angstrom, as for ``motion_correct_sum``.  With ``g = deformation_grid / float(pixel_spacing)`` (a torch
    op on the device) the result is ``correct_motion_fast(image, g).sum(0)``, or with ``dose_per_frame`` (e/A^2;
    with ``pre_exposure`` and ``voltage``) ``dose_weighted_sum(correct_motion_fast(image, g), pixel_spacing,
    dose_per_frame, pre_exposure, voltage)``.  ``return_plain_sum`` (needs a dose) returns ``(dose-weighted sum,
    plain sum)`` from the same pass.  The caller's grid is never modified.

    The example passes its Angstrom field straight to ``correct_motion_fast``, which reads the values as pixels;
    its literal result is ``motion_correct_sum_fast(img, field * ps, ps, ...)``.

    Both sums are linear: each frame is transformed forward once, its phase ramp applied and the sums accumulated
    in the forward column pass (engine.fast_shift_sums), then one inverse transform per sum -- no shifted frame
    is stored.  Frame shapes outside the row-major transforms (engine._full_row_major_ok) take exactly the
    composition above.  A field with more than one patch raises ValueError, as correct_motion_fast does."""
    dose = _check_fast_sum_args(dose_per_frame, return_plain_sum)  # every argument rule before any device
    if image.dim() != 3:
        raise ValueError(f"image must be (t, h, w), got {tuple(image.shape)}")
    _check_fast_field(deformation_grid, image.shape[0])
    want_plain = bool(return_plain_sum)
    with gpu_entry(image, device) as (out_dev, dev):
        sums = _fast_sums(_stage(image, dev), deformation_grid.detach().to(dev),
                          (float(pixel_spacing), dose, pre_exposure, voltage, want_plain))
        return _fast_result(sums, want_plain, out_dev)


def _check_raw_args(movie, gain):
    if movie.dim() != 3:
        raise ValueError(f"movie must be (t, h, w), got {tuple(movie.shape)}")
    if gain is not None and tuple(gain.shape) != tuple(movie.shape[-2:]):
        raise ValueError(f"gain reference has shape {tuple(gain.shape)}, frames are {tuple(movie.shape[-2:])}")


def motion_correct_sum_fast_raw(movie, gain, deformation_grid, pixel_spacing, mean_zero=True, hot_pixel_threshold=None,
                                dose_per_frame=None, pre_exposure=0.0, voltage=300.0, return_plain_sum=False,
                                device=None):
    """``motion_correct_sum_fast(condition_movie(movie, gain, mean_zero, hot_pixel_threshold), ...)`` for a RAW
    uint8 / int16 movie, without the conditioned movie: the row transform reads the raw bytes and forms
    ``raw * gain - frame mean`` as condition_movie rounds it, and the hot pixels (``hot_pixel_threshold``, the
    example uses 10.0) enter the spectra as sparse corrections (engine.RawMovie).  Without hot pixels the sums are
    bit for bit those of the conditioned route.  Returns the sum, or ``(dose-weighted sum, plain sum)`` with
    ``return_plain_sum``.  fp16 / fp32 movies, frame shapes outside the row-major transforms and a hot-pixel list
    overflow take exactly condition_movie followed by motion_correct_sum_fast."""
    dose = _check_fast_sum_args(dose_per_frame, return_plain_sum)  # every argument rule before any device
    thr = engine.check_hot_pixel_threshold(hot_pixel_threshold)
    _check_raw_args(movie, gain)
    _check_fast_field(deformation_grid, movie.shape[0])
    want_plain = bool(return_plain_sum)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, gd = _stage_raw(movie, gain, dev)
        ps = float(pixel_spacing)
        field = deformation_grid.detach().to(dev)
        sums = (ps, dose, pre_exposure, voltage, want_plain)
        res, _ = _raw_or_conditioned(
            raw, gd, mean_zero, thr=thr,
            fused=lambda rm: engine.fast_shift_sums(rm, engine.fast_shifts(field / ps), *sums),
            conditioned=lambda img: _fast_sums(img, field, sums))
        return _fast_result(res, want_plain, out_dev)


def motion_correct_raw_fast(movie, gain, pixel_spacing, reference_frame=None, b_factor=500, frequency_range=(300, 10),
                            mean_zero=True, hot_pixel_threshold=None, dose_per_frame=None, pre_exposure=0.0,
                            voltage=300.0, return_plain_sum=False, return_hot_counts=False, device=None):
    """The example's whole-image route for a RAW uint8 / int16 movie: condition_movie -> estimate_global_motion ->
    correct_motion_fast -> sum / dose_weight (examples/ttMotion.py:90-121, 174-199, 242-262, 390-404), with one
    engine.RawMovie for the estimate and the sums: no conditioned and no shifted fp32 movie.  Returns ``(field
    (2,t,1,1) Angstrom, sum (h,w)[, plain sum][, hot counts (t,) int32])``; the field is bit for bit
    ``motion_correct_raw``'s (the same estimator on the same RawMovie).  The sums are motion_correct_sum_fast's of
    the conditioned movie with that field (``correct_motion_fast`` with the field in pixels -- note the example
    itself passes the Angstrom field).  fp16 / fp32 movies, shapes without the fused kernels and a hot-pixel list
    overflow take exactly condition_movie, estimate_global_motion and motion_correct_sum_fast."""
    dose = _check_fast_sum_args(dose_per_frame, return_plain_sum)  # every argument rule before any device
    thr = engine.check_hot_pixel_threshold(hot_pixel_threshold)
    _check_raw_args(movie, gain)
    want_plain, want_counts = bool(return_plain_sum), bool(return_hot_counts)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, gd = _stage_raw(movie, gain, dev)
        t = raw.shape[0]
        ref = t // 2 if reference_frame is None else int(reference_frame)
        ps = float(pixel_spacing)
        sums = (ps, dose, pre_exposure, voltage, want_plain)

        def route(estimate, fast_sums):  # the same steps on a RawMovie and on the conditioned movie
            def run(src):
                shifts = estimate(src, ref, ps, float(b_factor), tuple(frequency_range))
                field = image_shifts_to_deformation_field(shifts, ps)  # as motion_correct_raw
                return field, fast_sums(src, field)
            return run

        (field, (dw, plain)), counts = _raw_or_conditioned(
            raw, gd, mean_zero, thr=thr,
            fused=route(engine.global_shifts_raw,
                        lambda rm, f: engine.fast_shift_sums(rm, engine.fast_shifts(f / ps), *sums)),
            conditioned=route(engine.global_shifts, lambda img, f: _fast_sums(img, f, sums)))
        out = [field.to(out_dev), (plain if dw is None else dw).to(out_dev)]
        if want_plain:
            out.append(plain.to(out_dev))
        if want_counts:
            out.append(_hot_counts_out(counts, t, out_dev))
        return tuple(out)


# ------------------------------------------------------------------ Fourier cropping (2x binning)


def _check_crop_args(shape, binning):
    """binning 2 and even frames (ValueError), frame sizes the cropping column pass takes (NotImplementedError naming
    them) -- all before any device is touched."""
    if isinstance(binning, bool) or binning != 2:
        raise ValueError(f"binning must be 2 (Fourier cropping by 2 per axis is the one factor built), got {binning!r}")
    h, w = int(shape[-2]), int(shape[-1])
    if h % 2 or w % 2 or h < 2 or w < 2:
        raise ValueError(f"Fourier cropping by 2 needs frames with an even number of rows and columns, got {h} x {w}")
    if not engine.fourier_crop_supported(h, w):
        raise NotImplementedError(f"frames of {h} x {w}: the Fourier crop needs {engine.FOURIER_CROP_SIZES}")


def fourier_crop(image, binning=2, device=None):
    """Fourier cropping ("Fourier binning", MotionCor's ``-FtBin 2``) of a frame (h, w) or a stack (t, h, w), fp32 or
    fp16, to (h/2, w/2): per frame ``irfft2(cat(F[:h/4, :w/4+1], F[h-h/4:, :w/4+1]), s=(h/2, w/2))`` of
    ``F = rfft2(frame)`` -- the signed row frequencies -h/4 <= ky < h/4 and columns kx <= w/4, the inverse's 1 /
    ((h/2)(w/2)) the only scale: an output pixel holds the counts of the 4 input pixels it stands for (a frame's sum
    is kept, a mean of zero stays zero).  A super-resolution movie, or a full-size sum of any function here, comes
    down to the detector's physical grid in one call.  Returns fp32 on ``image``'s device rule.  ``binning`` other
    than 2 and odd sizes raise ValueError; even sizes outside heights 512 .. 4096 (powers of two) / 8184 and widths
    128 .. 8192 (powers of two) / 11520 raise NotImplementedError (no chirp-z route, no CPU fallback)."""
    if not isinstance(image, torch.Tensor) or image.dim() not in (2, 3):
        raise ValueError(f"image must be (h, w) or (t, h, w), got {tuple(getattr(image, 'shape', ()))}")
    _check_crop_args(image.shape, binning)
    with gpu_entry(image, device) as (out_dev, dev):
        img = _stage(image, dev)
        out = engine.fourier_crop(img if img.dim() == 3 else img[None])
        return (out if img.dim() == 3 else out[0]).to(out_dev)


def _crop_raw(raw, gd, mean_zero, thr):
    """(binned fp32 movie, hot counts or None) of a movie on the device: engine.fourier_crop of the RawMovie, or of
    the conditioned movie."""
    return _raw_or_conditioned(raw, gd, mean_zero, thr=thr, fused=engine.fourier_crop, conditioned=engine.fourier_crop)


def fourier_crop_raw(movie, gain, binning=2, mean_zero=True, hot_pixel_threshold=None, return_hot_counts=False,
                     device=None):
    """``fourier_crop(condition_movie(movie, gain, mean_zero, hot_pixel_threshold))`` for a RAW uint8 / int16 movie
    without the full-size fp32 movie: the row transform reads the raw bytes and forms ``raw * gain - frame mean`` as
    condition_movie rounds it, and the hot pixels enter the spectra as sparse corrections (engine.RawMovie).  Without
    hot pixels the result is bit for bit that of the composition.  Returns the (t, h/2, w/2) fp32 movie, with
    ``return_hot_counts`` also the (t,) int32 hot pixels per frame (zeros without a threshold).  fp16 / fp32 movies
    and a hot-pixel list overflow take exactly condition_movie followed by fourier_crop.  Argument rules as
    ``fourier_crop``."""
    thr = engine.check_hot_pixel_threshold(hot_pixel_threshold)  # every argument rule before any device
    _check_raw_args(movie, gain)
    _check_crop_args(movie.shape, binning)
    want_counts = bool(return_hot_counts)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, gd = _stage_raw(movie, gain, dev)
        binned, counts = _crop_raw(raw, gd, mean_zero, thr=thr)
        if not want_counts:
            return binned.to(out_dev)
        return binned.to(out_dev), _hot_counts_out(counts, movie.shape[0], out_dev)


def motion_correct_raw_binned(movie, gain, pixel_spacing, binning=2, patch_sidelength=None, reference_frame=None,
                              b_factor=500, frequency_range=(300, 10), grid_type="catmull_rom", mean_zero=True,
                              hot_pixel_threshold=None, dose_per_frame=None, pre_exposure=0.0, voltage=300.0,
                              return_plain_sum=False, return_hot_counts=False, device=None):
    """A super-resolution session's first step as one call: ``fourier_crop_raw`` to the detector's physical grid,
    then the estimate and the aligned sum THERE.  ``pixel_spacing`` is that of the input movie; everything after the
    crop runs at ``binning * pixel_spacing`` and the returned field (Angstrom) and sums (h/2, w/2) belong to the
    binned movie.  With ``binned = fourier_crop_raw(movie, gain, binning, mean_zero, hot_pixel_threshold)`` and
    ``ps = binning * pixel_spacing`` the result is, bit for bit,

    * ``patch_sidelength=None``: ``field = estimate_global_motion(binned, ps, reference_frame, b_factor,
      frequency_range)`` and ``motion_correct_sum_fast(binned, field, ps, dose_per_frame, pre_exposure, voltage,
      return_plain_sum)`` -> ``(field, sum[, plain sum])``, as ``motion_correct_raw_fast`` returns them;
    * with a ``patch_sidelength`` (pixels of the binned movie): ``field, centres =
      estimate_motion_cross_correlation_patches(binned, ps, reference_frame, b_factor=b_factor,
      frequency_range=frequency_range, patch_sidelength=patch_sidelength)`` and ``motion_correct_sum(binned, field,
      ps, grid_type, dose_per_frame=..., pre_exposure=..., voltage=...)`` -> ``(field, centres, sum)``;
      ``return_plain_sum`` belongs to the whole-image route only.

    ``return_hot_counts`` appends the (t,) int32 hot pixels per frame.  Argument rules as ``fourier_crop_raw``."""
    dose = _check_fast_sum_args(dose_per_frame, return_plain_sum)  # every argument rule before any device
    thr = engine.check_hot_pixel_threshold(hot_pixel_threshold)
    _check_raw_args(movie, gain)
    _check_crop_args(movie.shape, binning)
    if patch_sidelength is not None:
        _check_patch_sidelength(patch_sidelength)
        if return_plain_sum:
            raise ValueError("return_plain_sum belongs to the whole-image route (patch_sidelength=None)")
    want_plain, want_counts = bool(return_plain_sum), bool(return_hot_counts)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, gd = _stage_raw(movie, gain, dev)
        binned, counts = _crop_raw(raw, gd, mean_zero, thr=thr)
        ps = binning * float(pixel_spacing)
        # the public functions themselves on the device-resident binned movie: the composition by construction
        if patch_sidelength is None:
            field = estimate_global_motion(binned, ps, reference_frame=reference_frame, b_factor=b_factor,
                                           frequency_range=frequency_range)
            sums = motion_correct_sum_fast(binned, field, ps, dose_per_frame=dose, pre_exposure=pre_exposure,
                                           voltage=voltage, return_plain_sum=want_plain)
            out = [field, *(sums if want_plain else (sums,))]
        else:
            field, centers = estimate_motion_cross_correlation_patches(
                binned, ps, reference_frame=reference_frame, b_factor=b_factor, frequency_range=frequency_range,
                patch_sidelength=int(patch_sidelength))
            out = [field, centers, motion_correct_sum(binned, field, ps, grid_type=grid_type, dose_per_frame=dose,
                                                      pre_exposure=pre_exposure, voltage=voltage)]
        if want_counts:
            out.append(_hot_counts_out(counts, movie.shape[0], dev))  # (moved to out_dev with the rest)
        return tuple(x.to(out_dev) for x in out)


# ------------------------------------------------------------------ Fourier cropping to a given size


def _check_crop_to_args(shape_in, shape):
    """Even frames and an even, positive (h2, w2) no larger than them (ValueError), a pair of shapes the cropping
    passes take (NotImplementedError naming them) -> (h2, w2) as ints -- all before any device is touched."""
    h, w = int(shape_in[-2]), int(shape_in[-1])
    try:
        h2, w2 = (operator.index(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"shape must be two integers (h2, w2), got {shape!r}") from None
    if h % 2 or w % 2 or h < 2 or w < 2:
        raise ValueError(f"Fourier cropping needs frames with an even number of rows and columns, got {h} x {w}")
    if h2 < 2 or w2 < 2:
        raise ValueError(f"shape must be positive, got {h2} x {w2}")
    if h2 % 2 or w2 % 2:
        raise ValueError(f"Fourier cropping needs an even number of rows and columns in shape, got {h2} x {w2}")
    if h2 > h or w2 > w:
        raise ValueError(f"shape {h2} x {w2} exceeds the frames, {h} x {w}: Fourier cropping only makes frames smaller")
    if not engine.fourier_crop_to_supported(h, w, h2, w2):
        raise NotImplementedError(f"frames of {h} x {w} to {h2} x {w2}: the Fourier crop needs "
                                  f"{engine.FOURIER_CROP_TO_SIZES}")
    return h2, w2


def fourier_crop_to(image, shape, device=None):
    """Fourier cropping of a frame (h, w) or a stack (t, h, w), fp32 or fp16, to ``shape = (h2, w2)``, both even, no
    larger than the frame: per frame ``irfft2(cat(F[:h2/2, :w2/2+1], F[h-h2/2:, :w2/2+1]), s=(h2, w2))`` of ``F =
    rfft2(frame)`` -- the signed row frequencies -h2/2 <= ky < h2/2 (the new Nyquist row from the negative side) and
    columns kx <= w2/2, the inverse's 1 / (h2 w2) the only scale: a frame's sum is kept.  MotionCor's ``-FtBin 1.5``
    or 3 of a super-resolution movie, 2 of a K3 counting-mode movie, 4/3 of a 4096-row sum; ``fourier_crop_shape``
    gives the shape for a factor, ``fourier_crop_pixel_spacing`` the pixel spacing of the result.  At (h/2, w/2) of a
    frame ``fourier_crop`` takes, this is ``fourier_crop``, bit for bit.  Returns fp32 on ``image``'s device rule.
    Odd or non-positive sizes and a shape beyond the frame raise ValueError; pairs outside heights 512 -> 384, 4096
    -> 3072, 4092 -> 2046, 8184 -> 5456 / 2728 and widths 64 .. 8192 (powers of two), 5760, 11520 -> any of those or
    2880, 3072, 3840, 7680 raise NotImplementedError (no chirp-z route, no CPU fallback)."""
    if not isinstance(image, torch.Tensor) or image.dim() not in (2, 3):
        raise ValueError(f"image must be (h, w) or (t, h, w), got {tuple(getattr(image, 'shape', ()))}")
    out_shape = _check_crop_to_args(image.shape, shape)
    with gpu_entry(image, device) as (out_dev, dev):
        img = _stage(image, dev)
        out = engine.fourier_crop_to(img if img.dim() == 3 else img[None], out_shape)
        return (out if img.dim() == 3 else out[0]).to(out_dev)


def fourier_crop_to_raw(movie, gain, shape, mean_zero=True, hot_pixel_threshold=None, return_hot_counts=False,
                        device=None):
    """``fourier_crop_to(condition_movie(movie, gain, mean_zero, hot_pixel_threshold), shape)`` for a RAW uint8 /
    int16 movie without the full-size fp32 movie, by ``fourier_crop_raw``'s rules: the row transform reads the raw
    bytes, the hot pixels enter the spectra as sparse corrections, and without hot pixels the result is bit for bit
    that of the composition.  Returns the (t, h2, w2) fp32 movie, with ``return_hot_counts`` also the (t,) int32 hot
    pixels per frame.  fp16 / fp32 movies and a hot-pixel list overflow take exactly condition_movie followed by
    fourier_crop_to.  There is no one-call binned pipeline at these factors: align the result with
    ``refine_global_motion`` / ``motion_correct_sum_fast`` at ``fourier_crop_pixel_spacing``.  Argument rules as
    ``fourier_crop_to``."""
    thr = engine.check_hot_pixel_threshold(hot_pixel_threshold)  # every argument rule before any device
    _check_raw_args(movie, gain)
    out_shape = _check_crop_to_args(movie.shape, shape)
    want_counts = bool(return_hot_counts)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, gd = _stage_raw(movie, gain, dev)
        crop = lambda src: engine.fourier_crop_to(src, out_shape)  # noqa: E731  (a RawMovie or the conditioned movie)
        cropped, counts = _raw_or_conditioned(raw, gd, mean_zero, thr=thr, fused=crop, conditioned=crop)
        if not want_counts:
            return cropped.to(out_dev)
        return cropped.to(out_dev), _hot_counts_out(counts, movie.shape[0], out_dev)


def fourier_crop_shape(h, w, binning):
    """The (h2, w2) ``fourier_crop_to`` takes for frames of (h, w) that lies nearest (h / binning, w / binning), for
    a factor >= 1: (4092, 5760, 2) -> (2046, 2880), (8184, 11520, 1.5) -> (5456, 7680).  NotImplementedError, listing
    the factors there are for that frame size, where no supported shape is within 0.5 % on both axes.  Plain Python:
    no device."""
    h, w = operator.index(h), operator.index(w)
    try:
        b = float(binning)
    except (TypeError, ValueError):
        raise ValueError(f"binning must be a number >= 1, got {binning!r}") from None
    if isinstance(binning, bool) or not (math.isfinite(b) and b >= 1.0):
        raise ValueError(f"binning must be a number >= 1, got {binning!r}")
    shapes = engine.fourier_crop_to_shapes(h, w)
    miss = lambda s: max(abs(s[0] * b / h - 1.0), abs(s[1] * b / w - 1.0))  # noqa: E731
    best = min(shapes, key=miss, default=None)
    if best is None or miss(best) > 0.005:
        factors = sorted({round(h / h2, 4) for h2, w2 in shapes if abs((h / h2) / (w / w2) - 1.0) <= 0.005})
        raise NotImplementedError(f"frames of {h} x {w} by {binning!r}: the Fourier crop has the factors "
                                  f"{', '.join(f'{f:g}' for f in factors) or 'none'} for this size; it takes "
                                  f"{engine.FOURIER_CROP_TO_SIZES}")
    return best


def fourier_crop_pixel_spacing(shape_in, shape_out, pixel_spacing):
    """(ps_y, ps_x) of a frame cropped from ``shape_in`` to ``shape_out`` (their last two entries): the field of view
    stays, so each axis' spacing grows by its own ratio, ``pixel_spacing * h / h2`` and ``pixel_spacing * w / w2``
    (4092 / 2046 = 5760 / 2880 = 2 exactly; 8184 / 5456 = 11520 / 7680 = 1.5)."""
    (h, w), (h2, w2) = (tuple(int(v) for v in s[-2:]) for s in (shape_in, shape_out))
    if min(h, w, h2, w2) < 1:
        raise ValueError(f"shapes must be positive, got {h} x {w} and {h2} x {w2}")
    ps = float(pixel_spacing)
    return ps * h / h2, ps * w / w2


# ------------------------------------------------------------------ frame groups (low-dose movies)


def _check_group_args(movie, group):
    """A (t, h, w) uint8 / int16 movie without an empty axis and a `group` its window sums exactly -> group as an
    int; ValueError otherwise (before any device is touched)."""
    if not isinstance(movie, torch.Tensor) or movie.dim() != 3 or min(movie.shape) < 1:
        raise ValueError(f"movie must be (t, h, w), got {tuple(getattr(movie, 'shape', ()))}")
    if movie.dtype not in RAW_DTYPES:
        raise ValueError(f"movie must be a uint8 or int16 tensor, got {movie.dtype}")
    return engine.check_group(group, movie.shape[0], movie.dtype)


def group_frames_raw(movie, group, device=None):
    """Rolling frame-group sums of a RAW uint8 / int16 (t, h, w) movie (MotionCor2 ``-Group``, RELION
    ``--group_frames``): the int16 (t, h, w) movie whose frame ``i`` is the sum of the frames ``max(0, i - lo) ..
    min(t - 1, i + hi)``, ``lo = (group - 1) // 2``, ``hi = group // 2`` -- the centred window of ``group`` frames,
    clipped at the ends of the movie; ``group=1`` widens the movie.  At 0.05 - 0.3 e/A^2 per frame a single frame's
    correlation peak drowns in noise; the estimators are then run on these sums.  ``(sum raw) * gain = sum (raw *
    gain)``, so the result is a raw movie for every ``*_raw*`` function, with the same gain -- 2 bytes per pixel and
    no fp32 copy (mc_raw_group_frames: one streaming pass).

    Exact integers.  A uint8 window may hold ``min(group, t) <= 128`` frames (255 * 128 fits int16), an int16 window
    32768; longer ones, a ``group`` that is not an int >= 1 and movies of any other type raise ValueError before any
    device is touched.  An int16 window sum outside [-32768, 32767] raises ValueError naming ``group`` (a device
    flag, the one device-to-host read)."""
    group = _check_group_args(movie, group)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, _ = _stage_raw(movie, None, dev)
        return engine.group_frames_raw(raw, group).to(out_dev)


def motion_correct_raw_grouped(movie, gain, pixel_spacing, group, patch_sidelength=None, reference_frame=None,
                               b_factor=500, frequency_range=(300, 10), grid_type="catmull_rom", mean_zero=True,
                               dose_per_frame=None, pre_exposure=0.0, voltage=300.0, return_plain_sum=False,
                               device=None):
    """Motion correction of a low-dose RAW uint8 / int16 movie: the estimate on the rolling sums of ``group``
    neighbouring frames, the sums from the individual frames.  With ``grouped = group_frames_raw(movie, group)`` the
    result is, bit for bit,

    * ``patch_sidelength=None``: the field ``motion_correct_raw_fast(grouped, gain, pixel_spacing, reference_frame,
      b_factor, frequency_range, mean_zero)`` returns and ``motion_correct_sum_fast_raw(movie, gain, field,
      pixel_spacing, mean_zero, None, dose_per_frame, pre_exposure, voltage, return_plain_sum)`` -> ``(field, sum[,
      plain sum])``;
    * with a ``patch_sidelength``: ``field, centres`` of ``motion_correct_raw_patches(grouped, gain, pixel_spacing,
      patch_sidelength, reference_frame, b_factor=b_factor, frequency_range=frequency_range, grid_type=grid_type,
      mean_zero=mean_zero)`` and ``motion_correct_sum_raw(movie, gain, field, pixel_spacing, grid_type, mean_zero,
      None, dose_per_frame, pre_exposure, voltage)`` -> ``(field, centres, sum)``; ``return_plain_sum`` belongs to
      the whole-image route only.

    A centred window of a steady drift averages to the frame's own shift, so the field of the grouped movie is applied
    to the frames as it is.  Argument rules as ``group_frames_raw`` and the composed functions, all before any device
    is touched; what those refuse on the device (McorrUnsupported for patch sizes without a kernel, ...) propagates.
    There is no hot-pixel step: hot pixels of a grouped movie need a rule of their own."""
    dose = _check_dose(dose_per_frame)  # every argument rule before any device
    group = _check_group_args(movie, group)
    _check_raw_args(movie, gain)
    p = None
    if patch_sidelength is not None:
        p = _check_patch_sidelength(patch_sidelength)
        if return_plain_sum:
            raise ValueError("return_plain_sum belongs to the whole-image route (patch_sidelength=None)")
    _check_fast_sum_args(dose, return_plain_sum)
    want_plain = bool(return_plain_sum)
    with gpu_entry(movie, device) as (out_dev, dev):
        raw, gd = _stage_raw(movie, gain, dev)
        t, h, w = raw.shape
        ps = float(pixel_spacing)
        grouped = engine.group_frames_raw(raw, group)
        # the sums: the public functions themselves on the device-resident movie (their argument rules pass by
        # construction, their results stay on `dev`)
        if p is None:
            ref = t // 2 if reference_frame is None else int(reference_frame)
            fused_sums = not engine.POLYPHASE_FOURIER_SHIFT and engine._full_row_major_ok(h, w)

            def estimate(shifts_of, fused):  # motion_correct_raw_fast's routes, without the sums of the grouped movie
                def run(src):
                    field = image_shifts_to_deformation_field(
                        shifts_of(src, ref, ps, float(b_factor), tuple(frequency_range)), ps)
                    if fused and not fused_sums:  # its fused sums refuse the shape: estimate on the conditioned movie
                        raise McorrUnsupported(f"no fused Fourier-shift sums for frames of {h} x {w}")
                    return field
                return run

            field, _ = _raw_or_conditioned(grouped, gd, mean_zero, thr=None,
                                           fused=estimate(engine.global_shifts_raw, True),
                                           conditioned=estimate(engine.global_shifts, False))
            sums = motion_correct_sum_fast_raw(raw, gd, field, pixel_spacing=ps, mean_zero=mean_zero,
                                               dose_per_frame=dose, pre_exposure=pre_exposure, voltage=voltage,
                                               return_plain_sum=want_plain)
            out = [field, *(sums if want_plain else (sums,))]
        else:
            # the public route itself on the device-resident grouped movie (its aligned sum of the groups is dropped):
            # which shapes take its fused kernels is decided there
            field, centers, _ = motion_correct_raw_patches(
                grouped, gd, ps, patch_sidelength=p, reference_frame=reference_frame, b_factor=b_factor,
                frequency_range=frequency_range, grid_type=grid_type, mean_zero=mean_zero)
            out = [field, centers, motion_correct_sum_raw(raw, gd, field, pixel_spacing=ps, grid_type=grid_type,
                                                          mean_zero=mean_zero, dose_per_frame=dose,
                                                          pre_exposure=pre_exposure, voltage=voltage)]
        return tuple(x.to(out_dev) for x in out)


def get_pixel_shifts(frame, pixel_spacing, frame_deformation_grid, pixel_grid=None):
    """(h,w,2) per-pixel shifts in px from a (2,G_h,G_w) Angstrom lattice
    (correct_motion.py:132-185).  `pixel_grid` (..., 2) holds the (y, x) pixel coordinates to
    evaluate at (correct_motion.py:167-168); the reference always passes the identity grid
    coordinate_grid((h,w)), which -- like None -- takes the tabulated kernel; any other grid is
    evaluated point by point (mc_pixel_shifts_at), result shape = pixel_grid's."""
    with gpu_entry(frame) as (out_dev, dev):
        h, w = frame.shape[-2:]
        lat = _stage(frame_deformation_grid, dev)
        if pixel_grid is not None:
            if pixel_grid.shape[-1] != 2:
                raise ValueError(f"pixel_grid must have shape (..., 2), got {tuple(pixel_grid.shape)}")
            grid = _stage(pixel_grid, dev)
            identity = tuple(grid.shape) == (h, w, 2) and bool(
                (grid[..., 0] == torch.arange(h, device=dev, dtype=torch.float32)[:, None]).all()
                and (grid[..., 1] == torch.arange(w, device=dev, dtype=torch.float32)[None, :]).all())
            if not identity:
                return engine.pixel_shifts_at(lat, h, w, float(pixel_spacing), grid).to(out_dev)
        out = engine.pixel_shifts(lat, h, w, float(pixel_spacing))
        return out.to(out_dev)
