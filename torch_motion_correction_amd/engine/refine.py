"""Iterative sub-pixel refinement of the whole-frame shifts and of the shifts per (frame, patch)."""

from __future__ import annotations

import math
import operator

import numpy as np
import torch

from .. import _lib, engine as E, lattice, plan as planmod
from .._lib import check, ptr, stream_ptr


# ------------------------------------------------------------------ iterative sub-pixel refinement


def check_refine_args(max_iterations, threshold, what=("max_iterations", "convergence_threshold"), min_iterations=1):
    """(iterations, threshold) of the refinement as (int, float); ValueError otherwise (before any device is
    touched): a whole number of iterations >= `min_iterations`, a finite threshold >= 0 (0 = never stop early)."""
    try:
        if isinstance(max_iterations, bool):
            raise TypeError
        n = operator.index(max_iterations)
    except TypeError:
        raise ValueError(f"{what[0]} must be an integer >= {min_iterations}, got {max_iterations!r}") from None
    if n < min_iterations:
        raise ValueError(f"{what[0]} must be an integer >= {min_iterations}, got {max_iterations!r}")
    try:
        thr = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"{what[1]} must be a finite number >= 0, got {threshold!r}") from None
    if not (math.isfinite(thr) and thr >= 0.0):
        raise ValueError(f"{what[1]} must be a finite number >= 0, got {threshold!r}")
    return n, thr


def refine_under_px(h, w):
    """The whole-pixel under-correction of the refinement's `cur` spectra (mc_xc_aligned_refs): the correlation map is
    translated by (c, c), so a converged peak lies at (c, c) instead of (0, 0) and its 3 x 3 neighbourhood inside the
    map.  16 lies inside the 64 rows per end the near-window search of 1024-row and taller maps visits; small frames
    take a quarter of their shorter side."""
    return max(1, min(16, h // 4, w // 4))


def _kept_frequencies(pl, dev):
    """(fy (nky,), fx (nkx,)): signed frequencies of the plan's kept bins in cycles/pixel, as LocalMotionProblem
    forms them for mc_local_loss_sums."""
    g = pl.geom

    def build():
        rows = np.concatenate([np.arange(g.kyp), np.arange(g.H - g.kyn, g.H)])
        kk = np.where(rows < (g.H + 1) // 2, rows, rows - g.H).astype(np.float32)
        fy = torch.from_numpy(kk * np.float32(1.0 / g.H)).to(dev)
        fx = torch.from_numpy(np.arange(g.nkx).astype(np.float32) * np.float32(1.0 / g.W)).to(dev)
        return fy, fx

    return E._cached(("kept_freqs", str(dev), g.H, g.W, g.nkx, g.kyp, g.kyn), build)


def refine_shifts_from_spectra(S, t, reference_frame, pl, start=None, max_iterations=10, threshold=0.01):
    """Iterative sub-pixel alignment on the filtered spectra S (t, nkx, nky, 2) of the global estimate: every frame
    against the mean of the OTHER aligned frames, until the shifts stop moving (csrc/xc_refine.hip has the
    definition).  `start`: (t, 2) px shifts, default the integer estimate against `reference_frame`
    (_shifts_from_spectra).  Per iteration: mc_xc_aligned_refs, K3/K4/K6 (_peaks with cur = G, ref = REF) and
    mc_xc_refine_update; no frame is read again.  Stops after the iteration whose max |r| is below `threshold` px
    (one host read of max |r| per iteration; none with threshold 0), at the latest after `max_iterations`.
    Returns ((t, 2) fp32 px shifts, the reference frame's row exactly 0; per-iteration max |r| as a CPU float
    tensor)."""
    lib = _lib.load()
    dev = S.device
    ref = _lib.normalize_frame_index(reference_frame, t)
    if t > E.REFINE_MAX_FRAMES:
        raise NotImplementedError(f"{t} frames: the refinement kernels take at most {E.REFINE_MAX_FRAMES}")
    if t == 1:
        return torch.zeros((1, 2), dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.float32)
    shifts = (E._shifts_from_spectra(S, t, reference_frame, pl) if start is None
              else start.detach().to(device=dev, dtype=torch.float32)).contiguous().clone()
    g = pl.geom
    fy, fx = _kept_frequencies(pl, dev)
    under = refine_under_px(g.H, g.W)
    G, REF = torch.empty_like(S), torch.empty_like(S)
    idx = E._cached(("refine_pairs", str(dev), t), lambda: torch.arange(t, device=dev, dtype=torch.int32))
    hist = torch.zeros(max_iterations, dtype=torch.float32, device=dev)
    st = stream_ptr(dev)
    done = 0
    for k in range(max_iterations):
        check(lib.mc_xc_aligned_refs(ptr(S), ptr(shifts), ptr(fy), ptr(fx), ptr(G), ptr(REF), t, g.nkx, g.nky, under,
                                     st), "mc_xc_aligned_refs")
        peaks, _, nb = E._peaks(G, idx, REF, idx, pl, want_nbhd=True)
        check(lib.mc_xc_refine_update(ptr(peaks), ptr(nb), ptr(shifts), ref, t, g.H, g.W, under, ptr(hist[k:k + 1]),
                                      st), "mc_xc_refine_update")
        done = k + 1
        if threshold > 0.0 and float(hist[k]) < threshold:
            break
    return shifts, hist[:done].cpu()


def global_shifts_refined(img, reference_frame, pixel_spacing, b_factor, frequency_range, start=None,
                          max_iterations=10, threshold=0.01):
    """global_shifts followed by refine_shifts_from_spectra on the same spectra (computed exactly as global_shifts
    computes them) -> ((t, 2) px, history)."""
    t, h, w = img.shape
    _lib.normalize_frame_index(reference_frame, t)  # IndexError before any launch
    pl = planmod.get_xc_plan(h, w, pixel_spacing, b_factor, frequency_range, img.device)
    S = E._global_spectra(img, pl)
    return refine_shifts_from_spectra(S, t, reference_frame, pl, start, max_iterations, threshold)


# ------------------------------------------------------------------ iterative sub-pixel patch alignment


def patch_origins(shape, p):
    """(cy, cx, origin): the patch estimator's centres and the (npatch, 2) int64 (y, x) corner of every patch's
    window, centre - p // 2, patches in row-major (gy, gx) order."""
    t, h, w = shape
    cy, cx = lattice.patch_grid_centers(t, h, w, p)
    origin = np.stack([np.repeat(cy - p // 2, len(cx)), np.tile(cx - p // 2, len(cy))], axis=1).astype(np.int64)
    return cy, cx, origin


def refine_window_offsets(start_px, shape, p):
    """The whole-pixel displacement o of every job's window for the (t, npatch, 2) start shifts `start_px` (px,
    (y, x); any device): per axis o = clamp(rint(s0), -origin, (h - p, w - p) - origin) with rint rounding halves
    to even, so that the window read at origin + o stays inside the frame.  No K1 needs the offset in coarser
    units than one sample (the raw and fp16 row passes load their sample pairs unaligned).  -> int64, same shape."""
    t, h, w = shape
    _, _, origin = patch_origins(shape, p)
    org = torch.as_tensor(origin, device=start_px.device)
    lo = (-org).to(torch.float32)
    hi = (torch.tensor([h - p, w - p], device=start_px.device) - org).to(torch.float32)
    s0 = start_px.detach().to(torch.float32).reshape(t, -1, 2)
    return torch.maximum(torch.minimum(torch.round(s0), hi), lo).to(torch.int64)


def start_field_px(field, pixel_spacing, t, gh, gw):
    """(t, gh * gw, 2) px start shifts from a (2, nt, nh, nw) Angstrom field on the device: resampled to
    (t, gh, gw) as resample_deformation_field does (Catmull-Rom) and divided by the pixel spacing (a device
    divisor: the correctly rounded quotient, see rigid_shifts_px)."""
    lin = lambda n: torch.linspace(0, 1, steps=n)  # noqa: E731
    lat = E.spline_lattice(field.to(torch.float32).contiguous(), lin(t), lin(gh), lin(gw), "catmull_rom")
    ps = torch.full((), float(pixel_spacing), dtype=torch.float32, device=lat.device)
    return torch.div(lat, ps).permute(1, 2, 3, 0).reshape(t, gh * gw, 2).contiguous()


def refine_patch_shifts(spectra, shape, pl, p, start_px, reference_frame, max_iterations=10, threshold=0.01):
    """Iterative sub-pixel alignment with one shift per (frame, patch): every patch of every frame against the mean
    of the same patch of the OTHER aligned frames (csrc/xc_refine_patches.hip has the definition), built like
    refine_shifts_from_spectra.  `spectra`: the K1 / K2 source of the patch estimator (_patch_spectra /
    _patch_spectra_raw); `start_px`: (t, npatch, 2) px on the device.  The windows are cut once, at the patch origin
    + refine_window_offsets(start_px), and transformed once (mask exponent 1); an iteration -- per chunk of
    patches mc_xc_aligned_refs_patches, K3/K4/K6 and mc_xc_refine_update_patches -- only touches those spectra.
    G' and REF hold one chunk of patches, at most WORKSPACE_BYTES each.  Stops after the iteration whose max |r|
    over all (frame, patch) is below `threshold` px (one host read per iteration; none with threshold 0), at the
    latest after `max_iterations`.  Returns ((t, npatch, 2) fp32 px shifts, row `reference_frame` exactly 0 in
    every patch; per-iteration max |r| as a CPU float tensor)."""
    lib = _lib.load()
    t, h, w = shape
    dev = start_px.device
    ref = _lib.normalize_frame_index(reference_frame, t)
    if t > E.REFINE_MAX_FRAMES:
        raise NotImplementedError(f"{t} frames: the refinement kernels take at most {E.REFINE_MAX_FRAMES}")
    _, _, origin = patch_origins(shape, p)
    npatch = origin.shape[0]
    if t == 1:
        return torch.zeros((1, npatch, 2), dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.float32)
    shifts = start_px.detach().to(torch.float32).reshape(t, npatch, 2).contiguous().clone()
    offs = refine_window_offsets(shifts, shape, p)
    corner = torch.as_tensor(origin[:, 0] * w + origin[:, 1], device=dev)
    frame0 = torch.arange(t, device=dev, dtype=torch.int64) * (h * w)
    job_off = (frame0[:, None] + corner[None, :] + offs[..., 0] * w + offs[..., 1]).reshape(-1).contiguous()
    ones = torch.ones(t * npatch, dtype=torch.int32, device=dev)
    S = spectra(job_off, ones, np.repeat(np.arange(t, dtype=np.int64), npatch), min_expo=1)
    offs = offs.to(torch.float32).contiguous()
    g = pl.geom
    fy, fx = _kept_frequencies(pl, dev)
    under = refine_under_px(g.H, g.W)
    nq, spans = E._chunks(npatch, t * g.nkx * g.nky * 8, most=65535)
    G = torch.empty((t * nq, g.nkx, g.nky, 2), dtype=torch.float32, device=dev)
    REF = torch.empty_like(G)
    idx = torch.arange(t * nq, device=dev, dtype=torch.int32)
    patch_max = torch.zeros(npatch, dtype=torch.float32, device=dev)
    hist = torch.zeros(max_iterations, dtype=torch.float32, device=dev)
    st = stream_ptr(dev)
    done = 0
    for k in range(max_iterations):
        for q0, n in spans:
            check(lib.mc_xc_aligned_refs_patches(ptr(S), ptr(shifts), ptr(offs), ptr(fy), ptr(fx), ptr(G), ptr(REF), t,
                                                 npatch, q0, n, g.nkx, g.nky, under, st), "mc_xc_aligned_refs_patches")
            peaks, _, nb = E._peaks(G, idx[:t * n], REF, idx[:t * n], pl, want_nbhd=True)
            check(lib.mc_xc_refine_update_patches(ptr(peaks), ptr(nb), ptr(shifts), ref, t, npatch, q0, n, g.H, g.W,
                                                  under, ptr(patch_max), st), "mc_xc_refine_update_patches")
        hist[k] = patch_max.max()
        done = k + 1
        if threshold > 0.0 and float(hist[k]) < threshold:
            break
    return shifts, hist[:done].cpu()


def _local_shifts_refined(shape, dev, pixel_spacing, patch_sidelength, field, reference_frame, b_factor,
                          frequency_range, max_iterations, threshold, spectra, default_start):
    """The body of local_shifts_refined / local_shifts_raw_refined.  `spectra(pl)`: the K1 / K2 source of the movie
    for the patch plan, made once the start is known; `default_start()`: ((t, 2) px, history) of the whole-frame
    refinement of the same movie, the start without a `field`."""
    t, h, w = shape
    _lib.normalize_frame_index(reference_frame, t)  # IndexError before any launch
    p = int(patch_sidelength)
    E._check_patch_args("mean_except_current", p, h, w)
    cy, cx, _ = patch_origins(shape, p)
    pl = planmod.get_xc_plan(p, p, pixel_spacing, b_factor, frequency_range, dev)
    gh, gw = len(cy), len(cx)
    centres = lattice.centers_tensor(t, cy, cx)
    if t == 1:
        return torch.zeros((1, gh, gw, 2), dtype=torch.float32, device=dev), torch.zeros(0), centres
    if field is None:
        rigid, _ = default_start()
        field = (rigid * pixel_spacing).transpose(0, 1)[:, :, None, None]
    start = start_field_px(field, pixel_spacing, t, gh, gw)
    shifts, hist = refine_patch_shifts(spectra(pl), tuple(shape), pl, p, start, reference_frame, max_iterations,
                                       threshold)
    return shifts.reshape(t, gh, gw, 2), hist, centres


def local_shifts_refined(img, pixel_spacing, patch_sidelength, field, reference_frame, b_factor, frequency_range,
                         max_iterations=10, threshold=0.01):
    """refine_patch_shifts on an fp32 / fp16 stack, normalised inside K1 with the central-box statistics of the stack
    as it is.  `field`: the (2, nt, nh, nw) Angstrom start field on the device, or None for the result of
    global_shifts_refined on the same stack at its default iteration settings.
    -> ((t, gh, gw, 2) px shifts, history, (t, gh, gw, 3) centres)."""
    return _local_shifts_refined(
        img.shape, img.device, pixel_spacing, patch_sidelength, field, reference_frame, b_factor, frequency_range,
        max_iterations, threshold, lambda pl: E._patch_spectra(img, pl, E.central_box_stats(img)),
        lambda: global_shifts_refined(img, reference_frame, pixel_spacing, b_factor, frequency_range))


def local_shifts_raw_refined(rm: "RawMovie", pixel_spacing, patch_sidelength, field, reference_frame, b_factor,
                             frequency_range, max_iterations=10, threshold=0.01):
    """local_shifts_refined of the conditioned movie straight from a RawMovie: 1024-px patches and no hot-pixel
    threshold; anything else raises McorrUnsupported before anything is launched (there is no silent fall-back).
    The default start is global_shifts_raw_refined on the same RawMovie."""
    E._local_raw_check(rm)
    dev = rm.raw.device
    _lib.normalize_frame_index(reference_frame, rm.shape[0])
    E._raw_patch_plan(rm.shape, dev, "mean_except_current", patch_sidelength, pixel_spacing, b_factor, frequency_range)
    return _local_shifts_refined(
        rm.shape, dev, pixel_spacing, patch_sidelength, field, reference_frame, b_factor, frequency_range,
        max_iterations, threshold, lambda pl: E._patch_spectra_raw(rm, pl),
        lambda: E.global_shifts_raw_refined(rm, reference_frame, pixel_spacing, b_factor, frequency_range))
