"""The patch estimator: the spectra of the patch jobs and the per-patch shift field."""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib, engine as E, lattice, plan as planmod
from .._lib import check, ptr, stream_ptr


# ------------------------------------------------------------------ a8: patch field


def patch_field(img, stats, pixel_spacing, reference_frame, reference_strategy, b_factor,
                frequency_range, patch_sidelength, sub_pixel_refinement, temporal_smoothing,
                smoothing_window_size, field0, outlier_rejection, outlier_threshold):
    """Per-patch shift field (2,t,gh,gw) in Angstrom, mean-subtracted, plus the patch
    centres (estimate_motion_xc.py:250-411).  `img` is the (already pre-corrected)
    stack; `stats` = central-box statistics to normalise with inside K1, or None when
    `img` is already normalised.  `field0` = prior field resampled to (2,t,gh,gw) or None."""
    t, h, w = img.shape
    dev = img.device
    p = int(patch_sidelength)
    _check_patch_args(reference_strategy, p, h, w)
    pl = planmod.get_xc_plan(p, p, pixel_spacing, b_factor, frequency_range, dev)
    spectra = _patch_spectra(img, pl, stats)
    return _patch_field_core((t, h, w), dev, pl, p, pixel_spacing, reference_frame, reference_strategy,
                             sub_pixel_refinement, temporal_smoothing, smoothing_window_size, field0,
                             outlier_rejection, outlier_threshold, spectra)


def _patch_spectra(img, pl, stats):
    """The K1 / K2 source of the patch estimators for an fp32 / fp16 (t, h, w) stack ->
    ``spectra(job_off, job_expo, frames, expo_b=None, min_expo=None)``, the filtered spectra of the jobs (a pair
    with `expo_b`).  `stats`: central-box statistics to normalise with inside K1, or None."""
    w = img.shape[2]
    if img.dtype != torch.float32 and not E._wave_rows_geometry(pl.geom):
        # fp16 frames are read natively by the 1024-px patch kernel only (BASELINE C5); any other
        # patch size goes through the workgroup / chirp-z kernels on a widened copy (the statistics
        # were taken from the fp16 bytes: identical values)
        img = img.float()
    src = [img]

    def spectra(off, ex, frames, expo_b=None, min_expo=None):
        try:
            return E._forward_spectra(src[0], off, w, ex, pl, stats, job_expo_b=expo_b, min_expo=min_expo)
        except _lib.McorrUnsupported:
            if src[0].dtype == torch.float32:
                raise
            src[0] = src[0].float()  # the C side has no fp16 kernel for this case after all: widen once
            return E._forward_spectra(src[0], off, w, ex, pl, stats, job_expo_b=expo_b, min_expo=min_expo)

    return spectra


def _check_patch_args(reference_strategy, p, h, w):
    if reference_strategy not in ("middle_frame", "mean_except_current"):
        raise ValueError(f"Unknown reference_strategy: {reference_strategy}")
    if p > h or p > w:
        raise ValueError(f"patch_sidelength {p} exceeds the frame size {h}x{w}")


def _patch_field_core(shape, dev, pl, p, pixel_spacing, reference_frame, reference_strategy, sub_pixel_refinement,
                      temporal_smoothing, smoothing_window_size, field0, outlier_rejection, outlier_threshold,
                      spectra):
    """The patch estimator after its K1 source is chosen: `spectra(job_off, job_expo, frames, expo_b, min_expo)`
    returns the filtered spectra of the jobs (a pair with `expo_b`); `frames` = each job's frame index."""
    lib = _lib.load()
    t, h, w = shape
    g = pl.geom
    cy, cx = lattice.patch_grid_centers(t, h, w, p)
    gh, gw = len(cy), len(cx)
    npatch = gh * gw
    origin = ((cy[:, None] - p // 2) * w + (cx[None, :] - p // 2)).reshape(-1)  # (npatch,)
    # the memo key is the caller's raw value (a negative key is an entry of its own in the
    # reference's memo, patch_grid/_patch_grid.py:283-294); the data come from the wrapped index
    ref_key = int(reference_frame)
    reference_frame = _lib.normalize_frame_index(ref_key, t)
    ref_expo, cur_expo, processed, ref_read = lattice.mask_schedule(t, reference_strategy, ref_key,
                                                                    with_ref_reads=True)
    field = torch.zeros((2, t, gh, gw), dtype=torch.float32, device=dev) if field0 is None \
        else field0.contiguous().clone()
    st = stream_ptr(dev)

    def jobs(frames, expos):
        off = (np.asarray(frames, dtype=np.int64)[:, None] * (h * w) + origin[None, :]).reshape(-1)
        ex = np.repeat(np.asarray(expos, dtype=np.int32), npatch)
        return E._i64(off, dev), E._i32(ex, dev), np.repeat(np.asarray(frames, dtype=np.int64), npatch)

    nproc = len(processed)
    if nproc > 0:
        if reference_strategy == "mean_except_current":
            if t < 2:
                raise ValueError("mean_except_current needs at least 2 frames")
            if ref_expo.max() > 1 or cur_expo.max() > 0:
                raise NotImplementedError("unexpected mask schedule")
            off, ex1, fr = jobs(range(t), [1] * t)
            U, V = spectra(off, ex1, fr, expo_b=ex1 * 2, min_expo=1)
            sp, si, sr = lattice.leave_one_out_schedule(ref_expo)
            sp, si, sr = E._i32(sp, dev), E._i32(si, dev), torch.as_tensor(sr, device=dev)
            REF = torch.empty_like(U)
            check(lib.mc_xc_ref_mean_except_current(ptr(U), ptr(V), ptr(sp), ptr(si), ptr(sr), ptr(REF),
                                                    t, npatch, g.nkx * g.nky, 1.0 / (t - 1), st),
                  "mc_xc_ref_mean_except_current")
            del V
            S_cur, S_ref = U, REF
        else:
            exl = [int(cur_expo[f]) + 1 for f in processed]
            off, ex, fr = jobs(processed, exl)
            S_cur = spectra(off, ex, fr, min_expo=min(exl))
            exl = [int(ref_read[f]) + 1 for f in processed]
            off, ex, fr = jobs([reference_frame] * nproc, exl)
            S_ref = spectra(off, ex, fr, min_expo=min(exl))
        pair_idx = torch.arange(nproc * npatch, device=dev, dtype=torch.int32)
        peaks, _, nb = E._peaks(S_cur, pair_idx, S_ref, pair_idx, pl, want_nbhd=sub_pixel_refinement)
        flags = (1 if sub_pixel_refinement else 0) | (2 if outlier_rejection else 0)
        check(lib.mc_field_accumulate(ptr(peaks), ptr(nb), ptr(E._i32(processed, dev)), nproc, npatch,
                                      p, t, float(pixel_spacing), float(outlier_threshold), flags,
                                      ptr(field), st), "mc_field_accumulate")
    window = 0
    if temporal_smoothing:
        window = int(smoothing_window_size)
        if window % 2 == 0:
            window += 1
        window = min(window, t)
        if window < 3:
            window = 0  # (an even window = t for even t < window|1 is what scipy gets, xc.py:506-529)
    out = torch.empty_like(field)
    check(lib.mc_field_smooth_center(ptr(field), ptr(out), t, npatch, window, 1, st),
          "mc_field_smooth_center")
    return out, lattice.centers_tensor(t, cy, cx)
