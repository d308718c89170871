"""Device-side pipelines on top of libmcorr (all tensors already on the GPU).

These functions only allocate buffers (torch caching allocator), build small index
tables and enqueue libmcorr kernels on the current stream; they never synchronise (one exception:
a RawMovie with a hot-pixel threshold reads the length of its hot-pixel list back).
"""

from __future__ import annotations

import ctypes as C
import math
import operator

import numpy as np
import torch

from . import _lib, lattice, plan as planmod, spline
from ._lib import check, ptr, stream_ptr

WORKSPACE_BYTES = 2 << 30  # soft cap for one transposed intermediate (T1 / T2)
FUSED_SEARCH = True  # near-window arg-max (mc_xc_correlate_argmax); False: full T2 + separate kernels


_CONST: dict = {}


def _cached(key, build):
    """Small device-resident index/tap tables, built once per (shape, device)."""
    v = _CONST.get(key)
    if v is None:
        if len(_CONST) > 512:
            _CONST.clear()
        v = _CONST[key] = build()
    return v


def _i32(a, device):
    return torch.as_tensor(np.asarray(a, dtype=np.int32), device=device)


def _i64(a, device):
    return torch.as_tensor(np.asarray(a, dtype=np.int64), device=device)


def _pow2(n):
    return n > 0 and (n & (n - 1)) == 0


def _chunks(n, item_bytes, most=None):
    """THE workspace rule: `n` items whose intermediates take `item_bytes` each are processed `chunk` at a time,
    as many as fit WORKSPACE_BYTES (read at call time; `most`: a further cap on the chunk), at least one
    -> (chunk, [(first, count), ...]).  The chunk size is result-bearing: it sets the summation order of the dose
    accumulators and the path _peaks takes."""
    chunk = max(1, min(n if most is None else min(n, most), WORKSPACE_BYTES // item_bytes))
    return chunk, [(a, min(chunk, n - a)) for a in range(0, n, chunk)]


# ------------------------------------------------------------------ statistics


STORE_F16, STORE_F32 = 2, 3  # MC_STORE_* of include/mcorr.h


def storage_of(img: torch.Tensor) -> int:
    """Frame storage type tag of the *_t entry points: fp32, or fp16 read straight from its bytes."""
    if img.dtype == torch.float32:
        return STORE_F32
    if img.dtype == torch.float16:
        return STORE_F16
    raise TypeError(f"frames must be float32 or float16 on the device, got {img.dtype}")


def central_box_stats(img: torch.Tensor, frac_low=0.25, frac_high=0.75) -> torch.Tensor:
    """(mean, 1/std, std) of the central box over all frames (utils.py:49-84); fp16 frames are read
    as they are (statistics of the fp32 up-cast)."""
    lib = _lib.load()
    t, h, w = img.shape
    hl, hu, wl, wu = int(frac_low * h), int(frac_high * h), int(frac_low * w), int(frac_high * w)
    acc = torch.empty(2, dtype=torch.float64, device=img.device)
    out3 = torch.empty(3, dtype=torch.float32, device=img.device)
    check(lib.mc_central_box_stats_t(ptr(img), storage_of(img), t, h, w, hl, hu, wl, wu, ptr(acc), ptr(out3),
                                     stream_ptr(img.device)), "mc_central_box_stats")
    return out3


def normalize(img: torch.Tensor, stats: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    out = torch.empty_like(img)
    check(lib.mc_normalize(ptr(img), ptr(out), img.numel(), ptr(stats), stream_ptr(img.device)),
          "mc_normalize")
    return out


# ------------------------------------------------------------------ spectra


def _k1(lib, g, dev, src, off, row_stride, expo, mask, stats, T1, tw_row, n, st):
    if planmod.native_rows(g):
        return lib.mc_xc_rows_forward(ptr(src), ptr(off), row_stride, ptr(expo), ptr(mask), ptr(stats),
                                      ptr(T1), ptr(tw_row), n, g, st)
    line, _ = planmod.line_plan(planmod.row_line_length(g.W), -1, dev,
                                keep=planmod.row_line_keep(g.W, g.nkx))  # output-pruned when that shrinks M
    return lib.mc_xcg_rows_forward(ptr(src), ptr(off), row_stride, ptr(expo), ptr(mask), ptr(stats),
                                   ptr(T1), ptr(tw_row), line, n, g, st)


def _k2(lib, g, dev, T1, filt, S, tw_col, n, st):
    if planmod.native_height(g.H):
        return lib.mc_xc_cols_forward(ptr(T1), ptr(filt), ptr(S), ptr(tw_col), n, g, st)
    line, _ = planmod.line_plan(g.H, -1, dev)
    return lib.mc_xcg_cols_forward(ptr(T1), ptr(filt), ptr(S), line, n, g, st)


def _wave_rows_geometry(g):
    """The geometry of the wave-per-row patch kernels (mc_xc_rows_forward_dual*): rows of 1024 samples.
    A shortcut: the authority is wave512_shape (csrc/xc_rows_fwd.hip)."""
    return g.W == 1024 and g.nkx <= 128 and g.ny % 8 == 0


def _wave512_ok(g, job_expo, use_mask, min_expo):
    """Patch rows of 1024 samples can take the wave-per-row K1 (mc_xc_rows_forward_dual):
    needs the mask and per-job exponents that are all >= 1 (`min_expo`, known on the host)."""
    return (_wave_rows_geometry(g) and use_mask and job_expo is not None
            and min_expo is not None and min_expo >= 1)


def _filtered_spectra(pl, dev, njobs, rows_pass, dual=False, use_filter=True):
    """THE K1 + K2 loop of the estimators -> S (njobs, nkx, nky, 2), or (S, Sb) with `dual`.  Per chunk of jobs
    (_chunks over the transposed intermediate T1, and T1b with `dual`) `rows_pass(a, n, T1, T1b)` enqueues the row
    pass of jobs a .. a+n-1 into T1 (chunk, nkx, ny, 2) (and T1b); the column pass (_k2) follows into S[a:a+n]."""
    lib = _lib.load()
    g = pl.geom
    S = torch.empty((njobs, g.nkx, g.nky, 2), dtype=torch.float32, device=dev)
    Sb = torch.empty_like(S) if dual else None
    chunk, spans = _chunks(njobs, g.nkx * g.ny * 8 * (2 if dual else 1))
    T1 = torch.empty((chunk, g.nkx, g.ny, 2), dtype=torch.float32, device=dev)
    T1b = torch.empty_like(T1) if dual else None
    filt = pl.filt if use_filter else None
    st = stream_ptr(dev)
    for a, n in spans:
        rows_pass(a, n, T1, T1b)
        check(_k2(lib, g, dev, T1, filt, S[a : a + n], pl.tw_col, n, st), "xc cols forward")
        if dual:
            check(_k2(lib, g, dev, T1b, filt, Sb[a : a + n], pl.tw_col, n, st), "xc cols forward")
    return (S, Sb) if dual else S


def _forward_spectra(src, job_off, row_stride, job_expo, pl, stats, use_mask=True, use_filter=True,
                     job_expo_b=None, min_expo=None):
    """K1+K2 for a list of jobs -> S (njobs, nkx, nky, 2).  With `job_expo_b` the rows are read
    once and transformed twice (mask^job_expo and mask^job_expo_b): returns (S_a, S_b)."""
    lib = _lib.load()
    g, dev = pl.geom, src.device
    dual = job_expo_b is not None
    wave = _wave512_ok(g, job_expo, use_mask, min_expo)
    if src.dtype != torch.float32 and not wave:
        raise _lib.McorrUnsupported("only the wave-per-row patch kernel reads fp16 frames: widen the stack first")
    if dual and not wave:  # no fused kernel for this shape: two ordinary passes
        return (_forward_spectra(src, job_off, row_stride, job_expo, pl, stats, use_mask, use_filter),
                _forward_spectra(src, job_off, row_stride, job_expo_b, pl, stats, use_mask, use_filter))
    st = stream_ptr(dev)

    def rows_pass(a, n, T1, T1b):
        off = job_off[a : a + n]
        expo = None if job_expo is None else job_expo[a : a + n]
        if wave:
            expo_b = job_expo_b[a : a + n] if dual else None
            check(lib.mc_xc_rows_forward_dual_t(ptr(src), storage_of(src), ptr(off), row_stride, ptr(expo),
                                                ptr(expo_b), ptr(pl.mask), ptr(stats), ptr(T1), ptr(T1b),
                                                ptr(pl.tw_row), n, g,
                                                ptr(pl.chord) if USE_ROW_CHORDS else None, st),
                  "mc_xc_rows_forward_dual")
        else:
            check(_k1(lib, g, dev, src, off, row_stride, expo, pl.mask if use_mask else None, stats, T1,
                      pl.tw_row, n, st), "xc rows forward")

    return _filtered_spectra(pl, dev, int(job_off.numel()), rows_pass, dual, use_filter)


def _peaks(S_cur, cur_idx, S_ref, ref_idx, pl, want_nbhd, shift_rows=None, n_shift_rows=0):
    """K3+K4(+K6) for all pairs -> peaks (npairs,) int32, shifts (npairs,2), nb or None.
    With `shift_rows` (int32, one row index per pair) the shifts are scattered into a zeroed
    (n_shift_rows, 2) table instead (rows no pair writes stay exactly zero)."""
    lib = _lib.load()
    g, dev = pl.geom, S_cur.device
    npairs = int(cur_idx.numel())
    peaks = torch.empty(npairs, dtype=torch.int32, device=dev)
    shifts = torch.empty((n_shift_rows if shift_rows is not None else npairs, 2), dtype=torch.float32,
                         device=dev)
    nb = torch.empty((npairs, 3, 3), dtype=torch.float32, device=dev) if want_nbhd else None
    chunk, spans = _chunks(npairs, g.nkx * g.H * 8)
    T2 = torch.empty((chunk, g.nkx, g.H, 2), dtype=torch.float32, device=dev)
    ngrp = g.H // g.RG
    pv = torch.empty(chunk * ngrp + chunk * g.H, dtype=torch.float32, device=dev)
    pi = torch.empty(chunk * ngrp + chunk + 1, dtype=torch.int32, device=dev)
    st = stream_ptr(dev)
    scale = 1.0 / (g.H * g.W)
    # near-window search (+ the 3x3 neighbourhood of the peak when asked): the full map (T2) is
    # a device-side fallback that normally never runs (mc_xc_correlate_argmax)
    fused = FUSED_SEARCH and planmod.native_rows(g) and planmod.native_height(g.H) and g.H >= 1024
    scatter = shift_rows is not None and fused and chunk >= npairs  # one call zeroes + fills the table
    if shift_rows is not None and not scatter:
        table, shifts = shifts, torch.empty((npairs, 2), dtype=torch.float32, device=dev)
    if fused:
        T2n = torch.empty((chunk, g.nkx, 2 * lib.mc_xc_near_rows(g), 2), dtype=torch.float32, device=dev)
    for a, n in spans:
        if fused:
            check(lib.mc_xc_correlate_argmax(ptr(S_cur), ptr(cur_idx[a : a + n]), ptr(S_ref),
                                             ptr(ref_idx[a : a + n]), ptr(T2), ptr(T2n), ptr(pv), ptr(pi),
                                             ptr(peaks[a : a + n]),
                                             ptr(shifts) if scatter else ptr(shifts[a : a + n]),
                                             ptr(shift_rows) if scatter else None,
                                             n_shift_rows if scatter else 0,
                                             ptr(nb[a : a + n]) if want_nbhd else None, ptr(pl.tw_col),
                                             ptr(pl.tw_row), scale, n, g, st), "mc_xc_correlate_argmax")
            continue
        if planmod.native_height(g.H):
            check(lib.mc_xc_cols_inverse(ptr(S_cur), ptr(cur_idx[a : a + n]), ptr(S_ref),
                                         ptr(ref_idx[a : a + n]), ptr(T2), ptr(pl.tw_col), scale, n, g,
                                         st), "mc_xc_cols_inverse")
        else:
            line, _ = planmod.line_plan(g.H, +1, dev)
            check(lib.mc_xcg_cols_inverse(ptr(S_cur), ptr(cur_idx[a : a + n]), ptr(S_ref),
                                          ptr(ref_idx[a : a + n]), None, ptr(T2), line, scale, n, g, st),
                  "mc_xcg_cols_inverse")
        if planmod.native_rows(g):
            check(lib.mc_xc_rows_inverse_argmax(ptr(T2), ptr(pv), ptr(pi), ptr(peaks[a : a + n]),
                                                ptr(shifts[a : a + n]), ptr(pl.tw_row), n, g, st),
                  "mc_xc_rows_inverse_argmax")
        else:
            line, _ = planmod.line_plan(planmod.row_line_length(g.W), +1, dev)
            check(lib.mc_xcg_rows_inverse(ptr(T2), ptr(pv), ptr(pi), ptr(peaks[a : a + n]),
                                          ptr(shifts[a : a + n]), None, None, 0, ptr(pl.tw_row), line, n,
                                          g, st), "mc_xcg_rows_inverse")
        if want_nbhd and planmod.native_rows(g):
            check(lib.mc_xc_peak_neighbourhood(ptr(T2), ptr(peaks[a : a + n]), ptr(nb[a : a + n]),
                                               ptr(pl.tw_row), n, g, st),
                  "mc_xc_peak_neighbourhood")
        elif want_nbhd:  # any other width: nine direct sums over the kept columns
            check(lib.mc_xcg_peak_neighbourhood(ptr(T2), ptr(peaks[a : a + n]), ptr(nb[a : a + n]), n, g, st),
                  "mc_xcg_peak_neighbourhood")
    if shift_rows is not None and not scatter:  # general path: scatter with torch
        table.zero_()
        table[shift_rows.long()] = shifts
        shifts = table
    return peaks, shifts, nb


# ------------------------------------------------------------------ a1: global shifts


def mask_spectrum(pl, dev):
    """Pruned spectrum of the plan's mask, (nkx, nky, 2): K1+K2 of an all-ones window.
    Built once per plan; used by the fused-statistics path (normalisation by linearity)."""
    if getattr(pl, "mhat", None) is None:
        g = pl.geom
        ones = torch.ones((g.H, g.W), dtype=torch.float32, device=dev)
        off = torch.zeros(1, dtype=torch.int64, device=dev)
        pl.mhat = _forward_spectra(ones, off, g.W, None, pl, None, use_filter=False)[0].contiguous()
    return pl.mhat


def _global_spectra(img, pl, after_k1=None):
    """Filtered pruned spectra of all frames, (t, nkx, nky, 2), with normalize_image's
    statistics gathered inside K1 whenever the central box lies in the region K1 reads
    (always for near-square frames); otherwise a separate statistics pass.  `after_k1()`, if
    given, is called right after K1 has been enqueued on the fused path (the movie pipeline
    records an event there); the other path never calls it.
    `half_ok` is a shortcut: the authority on the rows the wave-per-row K1 takes is k1_route (csrc/xc_rows_fwd.hip)."""
    lib = _lib.load()
    t, h, w = img.shape
    dev, g = img.device, pl.geom
    hl, hu, wl, wu = int(0.25 * h), int(0.75 * h), int(0.25 * w), int(0.75 * w)
    job_off = _cached(("frame_off", str(dev), t, h, w),
                      lambda: torch.arange(t, device=dev, dtype=torch.int64) * (h * w))
    fused = (planmod.native_rows(g) and planmod.native_height(g.H) and hl >= g.y0 and hu <= g.y0 + g.ny and wl >= g.x0
             and wu <= g.x1 and wl % 2 == 0 and wu % 2 == 0 and hu > hl and wu > wl)
    # fp16 frames are read as they are by the wave-per-row K1 (4096 columns); any other shape widens once
    half_ok = (img.dtype == torch.float16 and fused and w == 4096 and g.nkx <= 512 and g.ny % 8 == 0
               and wl % 256 == 0 and wu % 256 == 0 and img.data_ptr() % 16 == 0)
    if img.dtype != torch.float32 and not half_ok:
        img = img.float()
    if not fused:
        return _forward_spectra(img, job_off, w, None, pl, central_box_stats(img))
    st = stream_ptr(dev)
    mhat = mask_spectrum(pl, dev)
    # provisional mean m0 keeps the linear fix-up free of cancellation; any value near the
    # true mean does, so one row of frame 0's box is enough (one small workgroup)
    acc = torch.empty(128, dtype=torch.float64, device=dev)  # 64 x {sum, sumsq}
    m0 = torch.empty(3, dtype=torch.float32, device=dev)
    check(lib.mc_xc_provisional_mean_t(C.c_void_p(img.data_ptr() + img.element_size() * (hl * w + wl)),
                                       storage_of(img), wu - wl, ptr(m0), st), "mc_xc_provisional_mean")
    fix = torch.empty(2, dtype=torch.float32, device=dev)
    out3 = torch.empty(3, dtype=torch.float32, device=dev)
    T1 = torch.empty((t, g.nkx, g.ny, 2), dtype=torch.float32, device=dev)
    S = torch.empty((t, g.nkx, g.nky, 2), dtype=torch.float32, device=dev)
    try:
        check(lib.mc_xc_rows_forward_stats_t(ptr(img), storage_of(img), ptr(job_off), w, ptr(pl.mask), ptr(m0),
                                             ptr(T1), ptr(pl.tw_row), t, g, hl, hu, wl, wu, ptr(acc), ptr(fix),
                                             ptr(out3), ptr(_box_chords(pl, hl, hu, wl, wu)), st),
              "mc_xc_rows_forward_stats")
    except _lib.McorrUnsupported:
        # the C side decides which shapes read fp16 natively (row engine, alignment, geometry); the
        # predicate above is only a shortcut -- on disagreement widen once, as the warps do
        if img.dtype == torch.float32:
            raise
        del T1, S
        return _global_spectra(img.float(), pl, after_k1)
    if after_k1 is not None:
        after_k1()
    check(lib.mc_xc_cols_forward_fix(ptr(T1), ptr(pl.filt), ptr(S), ptr(pl.tw_col), t, g, ptr(fix),
                                     ptr(mhat), st), "mc_xc_cols_forward_fix")
    return S


def _os_env_flag(name, default):
    import os

    v = os.environ.get(name)
    return default if v is None else v not in ("0", "false", "no")


def _box_chords(pl, hl, hu, wl, wu):
    """The plan's per-row chord table if the statistics box lies inside the chords (it does for
    the reference's circular mask: the box corner is at 0.35 n from the centre, the soft edge ends
    at 0.375 n), else None: K1 then clamps to the support box only."""
    if pl.chord is None or not USE_ROW_CHORDS:
        return None
    key = ("chord_ok", id(pl), hl, hu, wl, wu)

    def build():
        c = pl.chord[hl:hu]
        return bool((c[:, 0] <= wl).all()) and bool((c[:, 1] + 4 >= wu).all())

    return pl.chord if _cached(key, build) else None


USE_ROW_CHORDS = _os_env_flag("MC_ROW_CHORDS", True)


def global_shifts(img, reference_frame, pixel_spacing, b_factor, frequency_range, after_k1=None):
    """Integer-pixel (t,2) shifts of every frame against `reference_frame`
    (estimate_motion_xc.py:57-123); the reference frame's row is exactly zero.
    `reference_frame` follows the reference's Python indexing (xc.py:101,107): a negative value
    selects from the end but never equals a loop index, so that frame is NOT skipped (it is
    correlated with itself); anything outside [-t, t) raises IndexError.  `after_k1`: see
    ``_global_spectra``."""
    t, h, w = img.shape
    dev = img.device
    pl = planmod.get_xc_plan(h, w, pixel_spacing, b_factor, frequency_range, dev)
    S = _global_spectra(img, pl, after_k1)
    return _shifts_from_spectra(S, t, reference_frame, pl)


def _shifts_from_spectra(S, t, reference_frame, pl):
    """K3 + K4 of the global estimate: every frame's filtered spectrum against the reference frame's."""
    dev = S.device
    ref = _lib.normalize_frame_index(reference_frame, t)
    skip = int(reference_frame) >= 0
    cur = [f for f in range(t) if not (skip and f == ref)]
    if not cur:
        return torch.zeros((t, 2), dtype=torch.float32, device=dev)
    cur_idx, ref_idx = _cached(
        ("global_pairs", str(dev), t, ref, skip),
        lambda: (_i32(cur, dev), _i32([ref] * len(cur), dev)))
    # pair p = frame cur[p]: its shift goes to row cur[p] of the (t, 2) table; the reference
    # frame's row is written by nobody and stays exactly zero
    _, shifts, _ = _peaks(S, cur_idx, S, ref_idx, pl, want_nbhd=False, shift_rows=cur_idx, n_shift_rows=t)
    return shifts


# ------------------------------------------------------------------ iterative sub-pixel refinement


REFINE_MAX_FRAMES = 512  # mc_xc_aligned_refs / mc_xc_refine_update


def check_refine_args(max_iterations, threshold, what=("max_iterations", "convergence_threshold"), min_iterations=1):
    """(iterations, threshold) of the refinement as (int, float); ValueError otherwise (before any device is
    touched): a whole number of iterations >= `min_iterations`, a finite threshold >= 0 (0 = never stop early)."""
    import operator

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

    return _cached(("kept_freqs", str(dev), g.H, g.W, g.nkx, g.kyp, g.kyn), build)


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
    if t > REFINE_MAX_FRAMES:
        raise NotImplementedError(f"{t} frames: the refinement kernels take at most {REFINE_MAX_FRAMES}")
    if t == 1:
        return torch.zeros((1, 2), dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.float32)
    shifts = (_shifts_from_spectra(S, t, reference_frame, pl) if start is None
              else start.detach().to(device=dev, dtype=torch.float32)).contiguous().clone()
    g = pl.geom
    fy, fx = _kept_frequencies(pl, dev)
    under = refine_under_px(g.H, g.W)
    G, REF = torch.empty_like(S), torch.empty_like(S)
    idx = _cached(("refine_pairs", str(dev), t), lambda: torch.arange(t, device=dev, dtype=torch.int32))
    hist = torch.zeros(max_iterations, dtype=torch.float32, device=dev)
    st = stream_ptr(dev)
    done = 0
    for k in range(max_iterations):
        check(lib.mc_xc_aligned_refs(ptr(S), ptr(shifts), ptr(fy), ptr(fx), ptr(G), ptr(REF), t, g.nkx, g.nky, under,
                                     st), "mc_xc_aligned_refs")
        peaks, _, nb = _peaks(G, idx, REF, idx, pl, want_nbhd=True)
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
    S = _global_spectra(img, pl)
    return refine_shifts_from_spectra(S, t, reference_frame, pl, start, max_iterations, threshold)


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
    if img.dtype != torch.float32 and not _wave_rows_geometry(pl.geom):
        # fp16 frames are read natively by the 1024-px patch kernel only (BASELINE C5); any other
        # patch size goes through the workgroup / chirp-z kernels on a widened copy (the statistics
        # were taken from the fp16 bytes: identical values)
        img = img.float()
    src = [img]

    def spectra(off, ex, frames, expo_b=None, min_expo=None):
        try:
            return _forward_spectra(src[0], off, w, ex, pl, stats, job_expo_b=expo_b, min_expo=min_expo)
        except _lib.McorrUnsupported:
            if src[0].dtype == torch.float32:
                raise
            src[0] = src[0].float()  # the C side has no fp16 kernel for this case after all: widen once
            return _forward_spectra(src[0], off, w, ex, pl, stats, job_expo_b=expo_b, min_expo=min_expo)

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
        return _i64(off, dev), _i32(ex, dev), np.repeat(np.asarray(frames, dtype=np.int64), npatch)

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
            sp, si, sr = _i32(sp, dev), _i32(si, dev), torch.as_tensor(sr, device=dev)
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
        peaks, _, nb = _peaks(S_cur, pair_idx, S_ref, pair_idx, pl, want_nbhd=sub_pixel_refinement)
        flags = (1 if sub_pixel_refinement else 0) | (2 if outlier_rejection else 0)
        check(lib.mc_field_accumulate(ptr(peaks), ptr(nb), ptr(_i32(processed, dev)), nproc, npatch,
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
    lat = spline_lattice(field.to(torch.float32).contiguous(), lin(t), lin(gh), lin(gw), "catmull_rom")
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
    if t > REFINE_MAX_FRAMES:
        raise NotImplementedError(f"{t} frames: the refinement kernels take at most {REFINE_MAX_FRAMES}")
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
    nq, spans = _chunks(npatch, t * g.nkx * g.nky * 8, most=65535)
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
            peaks, _, nb = _peaks(G, idx[:t * n], REF, idx[:t * n], pl, want_nbhd=True)
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
    _check_patch_args("mean_except_current", p, h, w)
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
        max_iterations, threshold, lambda pl: _patch_spectra(img, pl, central_box_stats(img)),
        lambda: global_shifts_refined(img, reference_frame, pixel_spacing, b_factor, frequency_range))


def local_shifts_raw_refined(rm: "RawMovie", pixel_spacing, patch_sidelength, field, reference_frame, b_factor,
                             frequency_range, max_iterations=10, threshold=0.01):
    """local_shifts_refined of the conditioned movie straight from a RawMovie: 1024-px patches and no hot-pixel
    threshold; anything else raises McorrUnsupported before anything is launched (there is no silent fall-back).
    The default start is global_shifts_raw_refined on the same RawMovie."""
    _local_raw_check(rm)
    dev = rm.raw.device
    _lib.normalize_frame_index(reference_frame, rm.shape[0])
    _raw_patch_plan(rm.shape, dev, "mean_except_current", patch_sidelength, pixel_spacing, b_factor, frequency_range)
    return _local_shifts_refined(
        rm.shape, dev, pixel_spacing, patch_sidelength, field, reference_frame, b_factor, frequency_range,
        max_iterations, threshold, lambda pl: _patch_spectra_raw(rm, pl),
        lambda: global_shifts_raw_refined(rm, reference_frame, pixel_spacing, b_factor, frequency_range))


# ------------------------------------------------------------------ a14/a16: spline lattice


def spline_lattice(field, ut, uy, ux, grid_type):
    """Evaluate the (c,nt,nh,nw) spline grid `field` on the tensor-product lattice
    ut x uy x ux (CPU float32 coordinate vectors in [0,1]) -> (c, NT, NY, NX)."""
    lib = _lib.load()
    dev = field.device
    c, nt, nh, nw = field.shape
    tabs = []
    for n, u in ((nt, ut), (nh, uy), (nw, ux)):
        u = u.detach().to(torch.float32).cpu().contiguous()

        def build(n=n, u=u):
            idx, wts = spline.axis_taps(n, u, grid_type)
            return idx.to(dev), wts.to(dev), int(u.numel())

        tabs.append(_cached(("taps", str(dev), n, grid_type, u.numpy().tobytes()), build))
    out = torch.empty((c, tabs[0][2], tabs[1][2], tabs[2][2]), dtype=torch.float32, device=dev)
    f = field.contiguous()
    check(lib.mc_spline_lattice(ptr(f), c, nt, nh, nw, ptr(tabs[0][0]), ptr(tabs[0][1]), tabs[0][2],
                                ptr(tabs[1][0]), ptr(tabs[1][1]), tabs[1][2], ptr(tabs[2][0]),
                                ptr(tabs[2][1]), tabs[2][2], ptr(out), stream_ptr(dev)),
          "mc_spline_lattice")
    return out


def spline_points(field, tyx, grid_type):
    """Evaluate the (c,nt,nh,nw) spline grid at (n, 3) points (t, y, x in [0,1], CPU float32) ->
    (n, c) on the device: ONE launch (tap tables per point built on the host)."""
    lib = _lib.load()
    dev = field.device
    c, nt, nh, nw = field.shape
    pts = tyx.detach().to(torch.float32).cpu().reshape(-1, 3)
    n = int(pts.shape[0])
    out = torch.empty((n, c), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    tabs = [spline.axis_taps(size, pts[:, a].contiguous(), grid_type) for a, size in enumerate((nt, nh, nw))]
    dt = [(i.to(dev), w.to(dev)) for i, w in tabs]
    f = field.contiguous()
    check(lib.mc_spline_points(ptr(f), c, nt, nh, nw, ptr(dt[0][0]), ptr(dt[0][1]), ptr(dt[1][0]), ptr(dt[1][1]),
                               ptr(dt[2][0]), ptr(dt[2][1]), n, ptr(out), stream_ptr(dev)), "mc_spline_points")
    return out


def frame_lattices(field, t, grid_type):
    """(t, 2, 10gh, 10gw) Angstrom lattices, one per frame time linspace(0,1,t)
    (correct_motion.py:57,67-72)."""
    _, _, gh, gw = field.shape
    lin = lambda n: _cached(("linspace", n), lambda: torch.linspace(0, 1, steps=n))
    lat = spline_lattice(field, lin(t), lin(10 * gh), lin(10 * gw), grid_type)
    return lat.permute(1, 0, 2, 3).contiguous()


# ------------------------------------------------------------------ a15/a17/a18: warp


RIGID_KERNEL_HOOK = None  # callable(fn) -> calls fn(); set by bench.py to time warp_rigid_dma alone


def rigid_shifts_px(lattices, pixel_spacing):
    """(t, 2) fp32 pixel shifts of the rigid warp from the (t, 2, GH, GW) Angstrom lattices of a (2, t, 1, 1)
    field: the lattice value over the pixel spacing, the correctly rounded fp32 quotient -- the rule of rigid_tail,
    of the general-field kernel and of the reference (a CPU tensor over a Python float).  The divisor is a device
    tensor: ATen divides a CUDA tensor by a Python scalar as a multiply by fp32(1 / ps), which is one ulp off for
    some shifts (ps = 0.83: -3 px becomes -3 - 2.4e-7, and pixel row 3 falls outside the frame).  No host
    synchronisation."""
    ps = torch.full((), float(pixel_spacing), dtype=torch.float32, device=lattices.device)
    return torch.div(lattices[:, :, 0, 0], ps).contiguous()


def _rigid_scratch(lib, t, h, w, dev):
    """The rigid warp's scratch buffer (weight tables of t frames of h x w)."""
    nbytes = C.c_int64(0)
    check(lib.mc_warp_rigid_scratch_bytes(t, h, w, C.byref(nbytes)), "mc_warp_rigid_scratch_bytes")
    return torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)


def _field_scratch(lib, t, h, w, GH, GW, dev):
    """The deformation-field warp's scratch buffer for (GH, GW) lattices."""
    nbytes = C.c_int64(0)
    check(lib.mc_warp_scratch_bytes(t, h, w, GH, GW, C.byref(nbytes)), "mc_warp_scratch_bytes")
    return torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)


def _sum_target(out_sum, want_sum, accumulate, h, w, dev):
    """Where a raw warp's frame sum goes: the caller's `out_sum` (with `accumulate` the kernel adds to what it
    holds), a new (h, w) buffer with `want_sum`, else None."""
    if accumulate and out_sum is None:
        raise ValueError("accumulate needs out_sum")
    if out_sum is not None:
        return out_sum
    return torch.empty((h, w), dtype=torch.float32, device=dev) if want_sum else None


def rigid_tables(img, lattices, pixel_spacing):
    """The per-frame weight tables of the rigid warp (rigid_base + rigid_weights: phase 1 of
    mc_warp_rigid_phase_t) enqueued on the CURRENT stream -> an opaque handle for
    ``warp(..., rigid=True, tables=handle)``.  The movie pipeline builds them on the estimator's
    stream, so that the warp stream carries nothing but the resampling launch."""
    lib = _lib.load()
    t, h, w = img.shape
    dev = img.device
    shifts_px = rigid_shifts_px(lattices, pixel_spacing)
    scratch = _rigid_scratch(lib, t, h, w, dev)
    # phase 1 never touches the frames (only their geometry matters): tagged fp32 so that fp16 stacks of
    # any row length get their tables here, whichever kernel resamples them later
    check(lib.mc_warp_rigid_phase_t(ptr(img), STORE_F32, t, h, w, ptr(shifts_px), ptr(scratch), None, None, 1,
                                    stream_ptr(dev)), "mc_warp_rigid_phase")
    return shifts_px, scratch


def rigid_tables_from_shifts(shifts, img_shape, pixel_spacing, grid_type):
    """The movie pipeline's tail in two launches (mc_rigid_tables_from_shifts): (t,2) px shifts of the global
    estimate -> ((2,t,1,1) Angstrom field, handle for ``warp(..., rigid=True, tables=handle)``); the same
    numbers as image_shifts_to_deformation_field + frame_lattices + rigid_tables, bit for bit."""
    lib = _lib.load()
    t, h, w = img_shape
    dev = shifts.device

    def build():
        lin = torch.linspace(0, 1, steps=t)
        it, wt = spline.axis_taps(t, lin, grid_type)
        _, w1 = spline.axis_taps(1, torch.linspace(0, 1, steps=10)[:1], grid_type)  # lattice point 0 of a 1-sample axis
        return it.to(dev), wt.to(dev), w1[0].contiguous().to(dev)

    idx_t, w_t, w1 = _cached(("rigid_tail_taps", str(dev), t, grid_type), build)
    field = torch.empty((2, t), dtype=torch.float32, device=dev)
    shifts_px = torch.empty((t, 2), dtype=torch.float32, device=dev)
    scratch = _rigid_scratch(lib, t, h, w, dev)
    check(lib.mc_rigid_tables_from_shifts(ptr(shifts.contiguous()), float(pixel_spacing), ptr(idx_t), ptr(w_t), ptr(w1),
                                          ptr(w1), t, h, w, ptr(field), ptr(shifts_px), ptr(scratch), stream_ptr(dev)),
          "mc_rigid_tables_from_shifts")
    return field[:, :, None, None], (shifts_px, scratch)


def warp(img, lattices, pixel_spacing, want_frames=True, want_sum=False, rigid=False, tables=None):
    """Resample every frame through its lattice; returns (frames or None, sum or None).
    rigid=True: the lattices come from a (2,nt,1,1) field, i.e. one shift per frame ->
    the separable rigid kernel (`tables`: the handle of an earlier ``rigid_tables`` call for
    the same stack and lattices; `lattices` may then be None)."""
    lib = _lib.load()
    t, h, w = img.shape
    dev = img.device
    if rigid and img.dtype == torch.float16 and (w % 8 or img.data_ptr() % 16):
        img = img.float()  # fp16 rows that are not whole 8-sample units: widened once
    frames = torch.empty((t, h, w), dtype=torch.float32, device=dev) if want_frames else None
    total = torch.empty((h, w), dtype=torch.float32, device=dev) if want_sum else None  # the kernels store it
    if rigid:
        if tables is None and RIGID_KERNEL_HOOK is not None:
            tables = rigid_tables(img, lattices, pixel_spacing)
        if tables is None:
            shifts_px = rigid_shifts_px(lattices, pixel_spacing)
            scratch = _rigid_scratch(lib, t, h, w, dev)
            args = (ptr(img), storage_of(img), t, h, w, ptr(shifts_px), ptr(scratch), ptr(frames), ptr(total))
            check(lib.mc_warp_rigid_phase_t(*args, 0, stream_ptr(dev)), "mc_warp_rigid")
            return frames, total
        shifts_px, scratch = tables
        args = (ptr(img), storage_of(img), t, h, w, ptr(shifts_px), ptr(scratch), ptr(frames), ptr(total))
        run = lambda: check(lib.mc_warp_rigid_phase_t(*args, 2, stream_ptr(dev)), "mc_warp_rigid_phase")
        if RIGID_KERNEL_HOOK is None:
            run()
        else:  # instrumentation: the hook brackets the resampling kernel alone (bench.py)
            RIGID_KERNEL_HOOK(run)
        return frames, total
    _, _, GH, GW = lattices.shape
    scratch = _field_scratch(lib, t, h, w, GH, GW, dev)
    rc = lib.mc_warp_frames_t(ptr(img), storage_of(img), t, h, w, ptr(lattices), GH, GW, float(pixel_spacing),
                              ptr(scratch), ptr(frames), ptr(total), stream_ptr(dev))
    if rc == -2 and img.dtype != torch.float32:
        # fp16 frames outside the LDS-staged kernel's shapes (row length not a multiple of 8, dense
        # lattice): widen once and take the fp32 kernels
        rc = lib.mc_warp_frames(ptr(img.float()), t, h, w, ptr(lattices), GH, GW, float(pixel_spacing),
                                ptr(scratch), ptr(frames), ptr(total), stream_ptr(dev))
    check(rc, "mc_warp_frames")
    return frames, total


def pixel_shifts(lattice, h, w, pixel_spacing):
    """(h,w,2) px shifts from one (2,GH,GW) Angstrom lattice (correct_motion.py:132-185)."""
    lib = _lib.load()
    dev = lattice.device
    _, GH, GW = lattice.shape
    scratch = _field_scratch(lib, 1, h, w, GH, GW, dev)
    out = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
    check(lib.mc_pixel_shifts(ptr(lattice.contiguous()), GH, GW, h, w, float(pixel_spacing),
                              ptr(scratch), ptr(out), stream_ptr(dev)), "mc_pixel_shifts")
    return out


def pixel_shifts_at(lattice, h, w, pixel_spacing, coords):
    """get_pixel_shifts at arbitrary (..., 2) yx pixel coordinates (the reference's `pixel_grid`
    argument, correct_motion.py:167-168) -> (..., 2) px."""
    lib = _lib.load()
    dev = lattice.device
    _, GH, GW = lattice.shape
    pts = coords.reshape(-1, 2).contiguous()
    out = torch.empty_like(pts)
    if pts.shape[0]:
        check(lib.mc_pixel_shifts_at(ptr(lattice.contiguous()), GH, GW, h, w, float(pixel_spacing), ptr(pts),
                                     pts.shape[0], ptr(out), stream_ptr(dev)), "mc_pixel_shifts_at")
    return out.reshape(coords.shape)


# ------------------------------------------------------------------ a19: Fourier shift


POLYPHASE_FOURIER_SHIFT = False  # tests: force the x-polyphase form on frames that do not need it


def _full_spectra_chunks(img, g, consume, polyphase=False):
    """THE unmasked full-spectrum loop of the pruned engine (K1 + K2: no mask, filter or statistics) behind the
    Fourier-shift and dose routines.  Per chunk of frames (_chunks; T1 and S together make the factor 2) the frames
    a .. a+n-1 of the fp32 stack `img` are transformed into S and ``consume(a, n, S, T1, off, src)`` follows; T1 is
    dead by then and free as T2.  `polyphase` (csrc/polyphase.hip): every frame enters as two jobs of (h, w/2), its
    even and its odd columns -- `src` is the chunk's de-interleaved (2n, h, w/2) stack, evens first, and S holds 2n
    spectra; otherwise `src` is `img`.  `g`: the full geometry of one job, `off`: the jobs' element offsets in
    `src`.  Returns T1."""
    lib = _lib.load()
    t, h, w = img.shape
    dev = img.device
    k = 2 if polyphase else 1  # jobs per frame
    wj = w // k
    tw_row, tw_col = planmod.get_twiddles(wj, dev), planmod.get_twiddles(h, dev)
    chunk, spans = _chunks(t, 2 * k * g.nkx * g.H * 8)
    T1 = torch.empty((k * chunk, g.nkx, g.ny, 2), dtype=torch.float32, device=dev)
    S = torch.empty((k * chunk, g.nkx, g.nky, 2), dtype=torch.float32, device=dev)
    st = stream_ptr(dev)
    for a, n in spans:
        if polyphase:
            src = torch.cat([img[a:a + n, :, 0::2], img[a:a + n, :, 1::2]], dim=0).contiguous()  # (2n, h, w/2)
            off = torch.arange(2 * n, device=dev, dtype=torch.int64) * (h * wj)
        else:
            src, off = img, torch.arange(a, a + n, device=dev, dtype=torch.int64) * (h * w)
        check(_k1(lib, g, dev, src, off, wj, None, None, None, T1, tw_row, k * n, st), "xc rows forward")
        check(_k2(lib, g, dev, T1, None, S, tw_col, k * n, st), "xc cols forward")
        consume(a, n, S, T1, off, src)
    return T1


def _polyphase_geometry(h, w, what):
    if w % 4:
        raise NotImplementedError(f"frames of {w} columns: the polyphase {what} needs a width divisible by 4")
    return planmod.full_geometry(h, w // 2)


def _fourier_shift_polyphase(img, shifts):
    """fourier_shift for frames whose full spectrum does not fit one row line (csrc/polyphase.hip):
    even and odd columns are transformed as two (h, w/2) frames, one pointwise pass applies the
    radix-2 butterfly + phase ramp + inverse butterfly, the halves go back and are interleaved."""
    lib = _lib.load()
    t, h, w = img.shape
    g = _polyphase_geometry(h, w, "Fourier shift")
    dev = img.device
    out = torch.empty_like(img)
    st = stream_ptr(dev)
    shifts = shifts.to(dev, torch.float32).contiguous()

    def consume(a, n, S, T1, off, sub):
        check(lib.mc_polyphase_fourier_shift(ptr(S), ptr(shifts[a:a + n]), n, g.nkx, h, w, st),
              "mc_polyphase_fourier_shift")
        res = _inverse_frames(lib, g, S, 2 * n, h, w // 2, dev, st, out=torch.empty_like(sub), off=off, T2=T1)
        out[a:a + n, :, 0::2] = res[:n]
        out[a:a + n, :, 1::2] = res[n:]

    _full_spectra_chunks(img, g, consume, polyphase=True)
    return out


FULL_ROW_MAJOR = True  # tests: False forces the pruned engine's transposed layout on power-of-two frames
DOSE_COLUMN_MAJOR = True  # tests / A-B: False feeds the exposure-weighted pass from the row-major spectra


def _full_row_major_ok(h, w):
    """Frames the row-major full-spectrum kernels (csrc/full_fft.hip, full_sums.hip) take: power-of-two rows and
    columns, and the K3 detector's 5760 / 11520 columns and 4092 / 8184 rows (mixed radix)."""
    rows_ok = (_pow2(w) and 64 <= w <= 8192) or w in (5760, 11520)
    cols_ok = (_pow2(h) and 256 <= h <= 4096) or h in (4092, 8184)
    return FULL_ROW_MAJOR and rows_ok and cols_ok


def _fourier_shift_row_major(img, shifts):
    """fourier_shift on power-of-two frames: rows forward -> (columns forward, phase ramp, columns
    inverse) in one in-place kernel -> rows inverse, the spectrum row-major throughout."""
    lib = _lib.load()
    t, h, w = img.shape
    dev = img.device
    pitch = lib.mc_full_spectrum_pitch(w)
    tw_row, tw_col = planmod.get_twiddles(w, dev), planmod.get_twiddles(h, dev)
    out = torch.empty_like(img)
    chunk, spans = _chunks(t, h * pitch * 8)
    S = torch.empty((chunk, h, pitch, 2), dtype=torch.float32, device=dev)
    st = stream_ptr(dev)
    shifts = shifts.to(dev, torch.float32).contiguous()
    for a, n in spans:
        off = torch.arange(a, a + n, device=dev, dtype=torch.int64) * (h * w)
        check(lib.mc_full_rows_forward(ptr(img), ptr(off), w, ptr(S), ptr(tw_row), n, h, w, pitch, st),
              "mc_full_rows_forward")
        check(lib.mc_full_cols_shift(ptr(S), ptr(shifts[a:a + n]), ptr(tw_col), 1.0 / (h * w), n, h, w, pitch, st),
              "mc_full_cols_shift")
        check(lib.mc_full_rows_inverse(ptr(S), ptr(out), ptr(off), w, ptr(tw_row), n, h, w, pitch, st),
              "mc_full_rows_inverse")
    return out


def _rows_forward(src, first, n, S):
    """mc_full_rows_forward of the fp32 frames first .. first+n-1 of `src` (t, h, w) into S (chunk, h, pitch, 2)."""
    lib = _lib.load()
    _, h, w = src.shape
    dev = src.device
    off = torch.arange(first, first + n, device=dev, dtype=torch.int64) * (h * w)
    check(lib.mc_full_rows_forward(ptr(src), ptr(off), w, ptr(S), ptr(planmod.get_twiddles(w, dev)), n, h, w,
                                   S.shape[2], stream_ptr(dev)), "mc_full_rows_forward")


def _row_major_sums(shape, dev, forward_rows, shifts=None, pixel_spacing=1.0, dose_per_frame=None, pre_exposure=0.0,
                    voltage=300.0, want_plain=False):
    """Frame sums on the row-major kernels with ONE inverse transform per sum.  Per chunk of frames (the
    WORKSPACE_BYTES rule) `forward_rows(a, n, S)` enqueues the row transforms of frames a .. a+n-1 into S (chunk, h,
    pitch, 2); the forward column pass (mc_full_cols_shift_sum) then multiplies each frame by its phase ramp
    (`shifts`, (t, 2) fp32 px; None: no ramp) and accumulates, in registers over the chunk's frames, the
    exposure-weighted sum (with `dose_per_frame`) and / or the plain sum (`want_plain`, with shifts only).  A caller
    that makes the frames on the fly (warp a chunk, transform it, drop it) never holds more than one chunk of them.
    Returns (dose-weighted sum or None, plain sum or None)."""
    lib = _lib.load()
    t, h, w = shape
    with_dose = dose_per_frame is not None
    pitch = lib.mc_full_spectrum_pitch(w)
    tw_row, tw_col = planmod.get_twiddles(w, dev), planmod.get_twiddles(h, dev)
    per_frame = h * pitch * 8
    # 4096 / 4092 rows: the column pass reads a column-major copy of the chunk's spectra (mc_full_transpose):
    # contiguous columns instead of 8 bytes of every 128-byte line -- 4.4 -> 3.6 ms per 40 x 4096^2 exposure-weighted
    # sum, 8.6 -> 7.4 ms per 40 x 4092 x 5760 with the copy's own read + write pass paid.  Not for 8184 rows (14.4 ->
    # 15.2 ms per 12 frames: that column kernel is bound by its radix-31 pass on 512-thread workgroups, not by how it
    # is fed).
    colmajor = DOSE_COLUMN_MAJOR and h in (4096, 4092)
    chunk, spans = _chunks(t, (2 if colmajor else 1) * per_frame)
    S = torch.empty((chunk, h, pitch, 2), dtype=torch.float32, device=dev)
    ST = torch.empty((chunk, w // 2 + 1, h, 2), dtype=torch.float32, device=dev) if colmajor else None
    sums = torch.empty((int(with_dose) + int(want_plain), h, pitch, 2), dtype=torch.float32, device=dev)
    A = sums[0] if with_dose else None
    P = sums[-1] if want_plain else None
    st = stream_ptr(dev)
    for a, n in spans:
        forward_rows(a, n, S)
        sum_args = (None if shifts is None else ptr(shifts[a:a + n]), n, a, t, ptr(A), ptr(P), ptr(tw_col), h, w,
                    pitch, float(pixel_spacing), float(pre_exposure), float(dose_per_frame) if with_dose else 0.0,
                    float(voltage), 1 if a == 0 else 0, 1 if a + n >= t else 0, 1.0 / (h * w), st)
        if colmajor:
            check(lib.mc_full_transpose(ptr(S), ptr(ST), n, h, w, pitch, st), "mc_full_transpose")
            check(lib.mc_full_cols_shift_sum_cm(ptr(ST), *sum_args), "mc_full_cols_shift_sum_cm")
        else:
            check(lib.mc_full_cols_shift_sum(ptr(S), *sum_args), "mc_full_cols_shift_sum")
    del S, ST
    n = sums.shape[0]
    out = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    off = torch.arange(n, device=dev, dtype=torch.int64) * (h * w)
    check(lib.mc_full_rows_inverse(ptr(sums), ptr(out), ptr(off), w, ptr(tw_row), n, h, w, pitch, st),
          "mc_full_rows_inverse")
    return (out[0] if with_dose else None), (out[-1] if want_plain else None)


def warp_dose_weighted_sum(img, lattices, pixel_spacing, rigid, dose_per_frame, pre_exposure, voltage):
    """correct_motion -> dose_weight -> sum (examples/ttMotion.py:318-351, 398) without the corrected
    movie in memory: on the row-major sizes (powers of two, the K3 formats) the frames are warped,
    transformed and weighted a chunk at a time (BASELINE C5: 60 x 8184 x 11520 -- 22.6 GB of
    corrected fp32 frames are never allocated); other sizes warp everything first."""
    t, h, w = img.shape
    if POLYPHASE_FOURIER_SHIFT or not _full_row_major_ok(h, w):
        frames, _ = warp(img, lattices, pixel_spacing, want_frames=True, want_sum=False, rigid=rigid)
        return dose_weighted_sum(frames, pixel_spacing, dose_per_frame, pre_exposure, voltage)

    def forward_rows(a, n, S):  # the chunk's warped frames are released on return, before the next chunk's warp
        frames = warp(img[a:a + n], lattices[a:a + n], pixel_spacing, want_frames=True, want_sum=False, rigid=rigid)[0]
        _rows_forward(frames, 0, n, S)

    return _row_major_sums(img.shape, img.device, forward_rows, pixel_spacing=pixel_spacing,
                           dose_per_frame=dose_per_frame, pre_exposure=pre_exposure, voltage=voltage)[0]


def fourier_shift(img, shifts):
    """irfft2(rfft2(img) * exp(-2 pi i (fy sy + fx sx))) per frame; shifts (t,2) px
    (correct_motion.py:484-496)."""
    lib = _lib.load()
    t, h, w = img.shape
    dev = img.device
    if POLYPHASE_FOURIER_SHIFT:
        return _fourier_shift_polyphase(img, shifts)
    if _full_row_major_ok(h, w):
        return _fourier_shift_row_major(img, shifts)
    try:
        g = planmod.full_geometry(h, w)
    except NotImplementedError:
        if w % 4 == 0 and w <= 16384 and h <= 8192:
            return _fourier_shift_polyphase(img, shifts)  # too wide for one row line: even / odd columns
        raise
    out = torch.empty_like(img)
    st = stream_ptr(dev)
    shifts = shifts.to(dev, torch.float32).contiguous()
    # T1 is dead after K2 and has the same footprint as T2: reuse it
    _full_spectra_chunks(img, g, lambda a, n, S, T1, off, _: _inverse_frames(
        lib, g, S, n, h, w, dev, st, shifts=shifts[a:a + n], out=out, off=off, T2=T1))
    return out


def _inverse_frames(lib, g, S, n, h, w, dev, st, shifts=None, out=None, off=None, T2=None):
    """irfft2 of n full spectra S (n, nkx, nky) of the pruned engine, each multiplied by its phase ramp (`shifts`
    (n, 2) fp32 px; None: zero shifts): the column inverse (mc_fourier_shift_cols_inverse on native heights,
    mc_xcg_cols_inverse otherwise) into T2 (n, nkx, H; default: a new buffer), then the row inverse
    (mc_xc_rows_inverse_store on native rows, mc_xcg_rows_inverse otherwise) into `out` at element offsets `off`
    (default: a new (n, h, w) tensor).  Returns out."""
    tw_row, tw_col = planmod.get_twiddles(w, dev), planmod.get_twiddles(h, dev)
    if out is None:
        out = torch.empty((n, h, w), dtype=torch.float32, device=dev)
        off = torch.arange(n, device=dev, dtype=torch.int64) * (h * w)
    idx = torch.arange(n, device=dev, dtype=torch.int32)
    if shifts is None:
        shifts = torch.zeros((n, 2), device=dev, dtype=torch.float32)
    if T2 is None:
        T2 = torch.empty((n, g.nkx, g.H, 2), dtype=torch.float32, device=dev)
    if planmod.native_height(g.H):
        check(lib.mc_fourier_shift_cols_inverse(ptr(S), ptr(idx), ptr(shifts), ptr(T2), ptr(tw_col),
                                                1.0 / (h * w), n, g, st), "mc_fourier_shift_cols_inverse")
    else:
        line, _ = planmod.line_plan(g.H, +1, dev)
        check(lib.mc_xcg_cols_inverse(ptr(S), ptr(idx), None, None, ptr(shifts), ptr(T2), line,
                                      1.0 / (h * w), n, g, st), "mc_xcg_cols_inverse")
    if planmod.native_rows(g):
        check(lib.mc_xc_rows_inverse_store(ptr(T2), ptr(out), ptr(off), w, ptr(tw_row), n, g, st),
              "mc_xc_rows_inverse_store")
    else:
        line, _ = planmod.line_plan(planmod.row_line_length(g.W), +1, dev)
        check(lib.mc_xcg_rows_inverse(ptr(T2), None, None, None, None, ptr(out), ptr(off), w,
                                      ptr(tw_row), line, n, g, st), "mc_xcg_rows_inverse")
    return out


def _dose_weighted_sum_polyphase(img, pixel_spacing, dose_per_frame, pre_exposure, voltage):
    """dose_weighted_sum for frames too wide for one row line: even / odd columns (csrc/polyphase.hip)."""
    lib = _lib.load()
    t, h, w = img.shape
    g = _polyphase_geometry(h, w, "form")
    dev = img.device
    A = torch.empty((2, g.nkx, g.nky, 2), dtype=torch.float32, device=dev)
    st = stream_ptr(dev)
    _full_spectra_chunks(img, g, lambda a, n, S, *_: check(
        lib.mc_polyphase_dose_accumulate(ptr(S), n, a, t, ptr(A), g.nkx, h, w, float(pixel_spacing),
                                         float(pre_exposure), float(dose_per_frame), float(voltage),
                                         1 if a == 0 else 0, 1 if a + n >= t else 0, st),
        "mc_polyphase_dose_accumulate"), polyphase=True)
    halves = _inverse_frames(lib, g, A, 2, h, w // 2, dev, st)
    out = torch.empty((h, w), dtype=torch.float32, device=dev)
    out[:, 0::2] = halves[0]
    out[:, 1::2] = halves[1]
    return out


def dose_weighted_sum(img, pixel_spacing, dose_per_frame, pre_exposure=0.0, voltage=300.0):
    """sum_f irfft2(q_f * rfft2(frame_f)): the exposure-filtered frame sum of the reference's
    example pipeline (examples/ttMotion.py:331-351, 398) with ONE inverse transform per movie:
    full spectra of a chunk of frames (K1+K2, no mask / filter) -> mc_dose_accumulate -> inverse
    column and row passes.  Semantics of the absent third-party filter: parity unpinned."""
    lib = _lib.load()
    t, h, w = img.shape
    dev = img.device
    if POLYPHASE_FOURIER_SHIFT:
        return _dose_weighted_sum_polyphase(img, pixel_spacing, dose_per_frame, pre_exposure, voltage)
    if _full_row_major_ok(h, w):
        return _row_major_sums(img.shape, dev, lambda a, n, S: _rows_forward(img, a, n, S),
                               pixel_spacing=pixel_spacing, dose_per_frame=dose_per_frame, pre_exposure=pre_exposure,
                               voltage=voltage)[0]
    try:
        g = planmod.full_geometry(h, w)
    except NotImplementedError:
        if w % 4 == 0 and w <= 16384 and h <= 8192:
            return _dose_weighted_sum_polyphase(img, pixel_spacing, dose_per_frame, pre_exposure, voltage)
        raise
    A = torch.empty((1, g.nkx, g.nky, 2), dtype=torch.float32, device=dev)
    st = stream_ptr(dev)
    T1 = _full_spectra_chunks(img, g, lambda a, n, S, *_: check(
        lib.mc_dose_accumulate(ptr(S), n, a, t, ptr(A), w, h, float(pixel_spacing), float(pre_exposure),
                               float(dose_per_frame), float(voltage), 1 if a == 0 else 0, 1 if a + n >= t else 0, st),
        "mc_dose_accumulate"))
    # inverse of the single accumulated spectrum: Fourier-shift path with a zero shift
    T2 = T1[:1] if g.ny == g.H else None
    return _inverse_frames(lib, g, A, 1, h, w, dev, st, T2=T2)[0]


_RAW_KINDS = {torch.uint8: 0, torch.int16: 1, torch.float16: 2, torch.float32: 3}


# ------------------------------------------------------------------ N2: the rigid path straight from raw frames


def check_hot_pixel_threshold(thr):
    """None, or a finite threshold > 0 as a float; ValueError otherwise (before anything is launched)."""
    if thr is None:
        return None
    try:
        v = float(thr)
    except (TypeError, ValueError):
        raise ValueError(f"hot_pixel_threshold must be a finite number > 0, got {thr!r}") from None
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"hot_pixel_threshold must be a finite number > 0, got {thr!r}")
    return v


def hot_list_capacity(t, h, w):
    """Entries of a RawMovie's hot-pixel list: one per 4096 samples of the movie, at least 4096 (16 bytes each:
    2.6 MB for 40 x 4096^2).  A threshold that finds more hot pixels raises McorrUnsupported."""
    return max(4096, (t * h * w) // 4096)


class RawMovie:
    """A raw detector movie with what the fused kernels need to condition it on the fly
    (c = raw * gain - mu_f, examples/ttMotion.py:90-121, 180-199): the (t,h,w) u8 / i16 stack, the (h,w)
    fp32 gain reference and, from ONE pass over the raw bytes (mc_raw_movie_stats), the frame means `mu`,
    the per-frame offsets `sub` = mu + box mean and `mean_rstd` of the conditioned central box.  No fp32
    movie is ever allocated.

    With `hot_pixel_threshold` the hot-pixel step of examples/ttMotion.py:127-172 (the rule of
    condition_movie's, mc_condition_movie_hot) sits between the gain and the mean: a statistics pass that also
    sums v^2 over the whole frame and a detection pass (mc_raw_hot_detect) give the list of hot pixels --
    `hot_keys` (n,) int64 = f*h*w + pixel index, ascending, `hot_rv` (n, 2) = {replacement, value} -- and
    `hot_counts` (t,) int32; the statistics are those of the frames after replacement.  global_shifts_raw and
    warp_rigid_raw apply the list as sparse corrections.  Reading the list's length back costs one small
    device-to-host copy; more hot pixels than hot_list_capacity() raise McorrUnsupported."""

    def __init__(self, raw, gain, mean_zero=True, hot_pixel_threshold=None):
        thr = check_hot_pixel_threshold(hot_pixel_threshold)
        lib = _lib.load()
        if raw.dtype not in (torch.uint8, torch.int16):
            raise TypeError(f"the fused raw path reads uint8 or int16 frames, got {raw.dtype}")
        t, h, w = raw.shape
        dev = raw.device
        self.raw = raw.contiguous()
        self.gain = (torch.ones((h, w), dtype=torch.float32, device=dev) if gain is None
                     else gain.detach().to(device=dev, dtype=torch.float32).contiguous())
        if tuple(self.gain.shape) != (h, w):
            raise ValueError(f"gain reference {tuple(self.gain.shape)} does not match the frames {(h, w)}")
        self.kind = _RAW_KINDS[raw.dtype]
        self.shape = (t, h, w)
        self.hot_pixel_threshold = thr
        self.n_hot = 0
        self.hot_keys = self.hot_rv = self.hot_counts = None
        hl, hu, wl, wu = int(0.25 * h), int(0.75 * h), int(0.25 * w), int(0.75 * w)  # utils.py:76-81
        self.stats = torch.empty((t, 3), dtype=torch.float64, device=dev)
        self.mu = torch.empty(t, dtype=torch.float32, device=dev)
        self.sub = torch.empty(t, dtype=torch.float32, device=dev)
        self.mean_rstd = torch.empty(2, dtype=torch.float32, device=dev)
        st = stream_ptr(dev)
        if thr is None:
            check(lib.mc_raw_movie_stats(ptr(self.raw), self.kind, ptr(self.gain), t, h, w, hl, hu, wl, wu,
                                         1 if mean_zero else 0, ptr(self.stats), ptr(self.mu), ptr(self.sub),
                                         ptr(self.mean_rstd), st), "mc_raw_movie_stats")
            return
        cap = hot_list_capacity(t, h, w)
        hstats = torch.empty((t, 3), dtype=torch.float64, device=dev)
        keys = torch.empty(cap, dtype=torch.int64, device=dev)
        rv = torch.empty((cap, 2), dtype=torch.float32, device=dev)
        counter = torch.empty(1, dtype=torch.int64, device=dev)
        self.hot_counts = torch.empty(t, dtype=torch.int32, device=dev)
        check(lib.mc_raw_hot_detect(ptr(self.raw), self.kind, ptr(self.gain), t, h, w, hl, hu, wl, wu, thr,
                                    ptr(self.stats), ptr(hstats), ptr(keys), ptr(rv), cap, ptr(counter),
                                    ptr(self.hot_counts), st), "mc_raw_hot_detect")
        n = int(counter.item())  # the one device-to-host copy of the hot-pixel step
        if n > cap:
            raise _lib.McorrUnsupported(
                f"hot_pixel_threshold={thr:g} finds {n} hot pixels in this movie, more than the {cap} entries "
                "of the fused path's hot-pixel list")
        self.hot_keys, order = torch.sort(keys[:n], stable=True)
        self.hot_rv = rv[:n][order].contiguous()
        self.n_hot = n
        check(lib.mc_raw_hot_finalize(ptr(self.hot_keys), ptr(self.hot_rv), n, t, h, w, hl, hu, wl, wu,
                                      1 if mean_zero else 0, ptr(hstats), ptr(self.stats), ptr(self.mu),
                                      ptr(self.sub), ptr(self.mean_rstd), st), "mc_raw_hot_finalize")

    def window(self, a, n):
        """Frames [a, a+n) as a RawMovie of their own, without a copy of the movie: views of raw / mu / sub /
        stats / hot_counts, the same gain and mean_rstd, and the hot pixels of those frames -- the slice of the
        sorted `hot_keys` in [a*h*w, (a+n)*h*w), rebased to the window's first frame.  The warps and their hot-pixel
        corrections (_warp_hot_correct) then work per window unchanged."""
        t, h, w = self.shape
        if not (0 <= a and n >= 1 and a + n <= t):
            raise ValueError(f"frame window [{a}, {a + n}) outside a movie of {t} frames")
        hw = h * w
        win = object.__new__(RawMovie)
        win.raw = self.raw[a:a + n]
        # the raw kernels read 16-byte units from the first frame's first byte (h*w % 64 == 0 on every
        # row-major shape, so every window of those is aligned)
        assert win.raw.data_ptr() % 16 == 0, "frame window not 16-byte aligned"
        win.gain, win.kind, win.shape = self.gain, self.kind, (n, h, w)
        win.hot_pixel_threshold = self.hot_pixel_threshold
        win.stats, win.mu, win.sub, win.mean_rstd = self.stats[a:a + n], self.mu[a:a + n], self.sub[a:a + n], self.mean_rstd
        win.n_hot = 0
        win.hot_keys = win.hot_rv = win.hot_counts = None
        if self.hot_counts is not None:
            win.hot_counts = self.hot_counts[a:a + n]
        if self.n_hot:
            if getattr(self, "_frame_starts", None) is None:  # one device-to-host copy per movie
                bounds = torch.arange(t + 1, device=self.raw.device, dtype=torch.int64) * hw
                self._frame_starts = torch.searchsorted(self.hot_keys, bounds).tolist()
            lo, hi = self._frame_starts[a], self._frame_starts[a + n]
            win.n_hot = hi - lo
            win.hot_keys = self.hot_keys[lo:hi] - a * hw
            win.hot_rv = self.hot_rv[lo:hi]
        return win

    def device_tensors(self):
        """Every device tensor a consumer on another stream reads (for record_stream)."""
        return [x for x in (self.raw, self.gain, self.mu, self.sub, self.mean_rstd, self.hot_keys, self.hot_rv,
                            self.hot_counts) if x is not None]


def raw_fused_supported(raw, pl):
    """Shapes the fused raw kernels take (a shortcut: the C side is the authority and answers
    MC_ERR_UNSUPPORTED for anything else; the caller then conditions the movie into an fp32 copy).  K1 from
    raw bytes exists for power-of-two widths (4096: the wave-per-row engine) and the K3 formats' rows of 5760 /
    11520 samples; the raw warp needs rows of whole quads and at most 256 frames."""
    t, h, w = raw.shape
    g = pl.geom
    rows_ok = planmod.native_rows(g) or (w % 2 == 0 and planmod.row_line_length(w) in (2880, 5760)
                                        and planmod.USE_DIRECT_LINES)
    return raw.dtype in (torch.uint8, torch.int16) and rows_ok and w % 4 == 0 and t <= 256 and raw.data_ptr() % 16 == 0


def global_shifts_raw(rm: RawMovie, reference_frame, pixel_spacing, b_factor, frequency_range, after_k1=None):
    """global_shifts for a RawMovie: K1 reads the raw bytes (mc_xc_rows_forward_raw / mc_xcg_rows_forward_raw), the
    statistics are known beforehand, so the plain column pass follows.  Raises McorrUnsupported for shapes
    without a fused kernel.  `after_k1()`, if given, is called once the last chunk's K1 (and hot-pixel fix-up)
    has been enqueued."""
    S, pl = _global_spectra_raw(rm, reference_frame, pixel_spacing, b_factor, frequency_range, after_k1)
    return _shifts_from_spectra(S, rm.shape[0], reference_frame, pl)


def _global_spectra_raw(rm, reference_frame, pixel_spacing, b_factor, frequency_range, after_k1=None):
    """The filtered pruned spectra of global_shifts_raw and their plan -> (S (t, nkx, nky, 2), plan)."""
    lib = _lib.load()
    t, h, w = rm.shape
    dev = rm.raw.device
    _lib.normalize_frame_index(reference_frame, t)  # IndexError before any launch, as the fp32 path
    pl = planmod.get_xc_plan(h, w, pixel_spacing, b_factor, frequency_range, dev)
    g = pl.geom
    if not raw_fused_supported(rm.raw, pl):
        raise _lib.McorrUnsupported("no fused raw kernel for this frame shape")
    st = stream_ptr(dev)
    job_off = _cached(("frame_off", str(dev), t, h, w),
                      lambda: torch.arange(t, device=dev, dtype=torch.int64) * (h * w))
    chord = ptr(pl.chord) if (pl.chord is not None and USE_ROW_CHORDS) else None

    # row pass in chunks of frames when the transposed intermediate would be large (K3 formats: 0.4 GB per 10 frames)
    def rows_pass(a, n, T1, T1b):
        off, sub = job_off[a:a + n], rm.sub[a:a + n]
        if planmod.native_rows(g):
            check(lib.mc_xc_rows_forward_raw(ptr(rm.raw), rm.kind, ptr(rm.gain), ptr(off), w, ptr(pl.mask), ptr(sub),
                                             ptr(rm.mean_rstd), ptr(T1), ptr(pl.tw_row), n, g, chord, st),
                  "mc_xc_rows_forward_raw")
        else:
            line, _ = planmod.line_plan(planmod.row_line_length(g.W), -1, dev, keep=planmod.row_line_keep(g.W, g.nkx))
            check(lib.mc_xcg_rows_forward_raw(ptr(rm.raw), rm.kind, ptr(rm.gain), ptr(off), w, ptr(pl.mask), ptr(sub),
                                              ptr(rm.mean_rstd), ptr(T1), ptr(pl.tw_row), line, n, g, st),
                  "mc_xcg_rows_forward_raw")
        if rm.n_hot:  # hot pixels of these frames: sparse correction of T1 (no fp32 movie)
            check(lib.mc_xc_rows_hot_correct(ptr(rm.hot_keys), ptr(rm.hot_rv), rm.n_hot, a, n, h, w, ptr(pl.mask),
                                             ptr(rm.mean_rstd), ptr(T1), g, st), "mc_xc_rows_hot_correct")
        if a + n >= t and after_k1 is not None:
            after_k1()

    return _filtered_spectra(pl, dev, t, rows_pass), pl


def global_shifts_raw_refined(rm: RawMovie, reference_frame, pixel_spacing, b_factor, frequency_range, start=None,
                              max_iterations=10, threshold=0.01):
    """global_shifts_raw followed by refine_shifts_from_spectra on the same spectra -> ((t, 2) px, history).  Raises
    McorrUnsupported for shapes without a fused raw kernel, as global_shifts_raw."""
    S, pl = _global_spectra_raw(rm, reference_frame, pixel_spacing, b_factor, frequency_range)
    return refine_shifts_from_spectra(S, rm.shape[0], reference_frame, pl, start, max_iterations, threshold)


def warp_rigid_raw(rm: RawMovie, lattices, pixel_spacing, want_frames=True, want_sum=False, tables=None,
                   out_sum=None, accumulate=False):
    """``warp(..., rigid=True)`` of the conditioned movie without materialising it (mc_warp_rigid_raw).
    `out_sum`: the (h, w) buffer the sum goes to (implies want_sum); with `accumulate` the sum is added to what it
    holds (mc_warp_rigid_raw_accumulate) -- the hot-pixel corrections of these frames too."""
    t, h, w = rm.shape
    dev = rm.raw.device
    total = _sum_target(out_sum, want_sum, accumulate, h, w, dev)
    lib = _lib.load()
    frames = torch.empty((t, h, w), dtype=torch.float32, device=dev) if want_frames else None
    entry = lib.mc_warp_rigid_raw_accumulate if accumulate else lib.mc_warp_rigid_raw
    if tables is None:
        shifts_px = rigid_shifts_px(lattices, pixel_spacing)
        scratch = _rigid_scratch(lib, t, h, w, dev)
        phase = 0
    else:
        shifts_px, scratch = tables
        phase = 2
    run = lambda: check(entry(ptr(rm.raw), rm.kind, ptr(rm.gain), ptr(rm.mu), t, h, w, ptr(shifts_px), ptr(scratch),
                              ptr(frames), ptr(total), phase, stream_ptr(dev)), "mc_warp_rigid_raw")
    if RIGID_KERNEL_HOOK is not None and phase == 2:
        RIGID_KERNEL_HOOK(run)
    else:
        run()
    if rm.n_hot:
        _warp_hot_correct(lib, rm, scratch, frames, total, stream_ptr(dev))
    return frames, total


def _local_raw_check(rm: RawMovie):
    if rm.hot_pixel_threshold is not None:
        raise _lib.McorrUnsupported("the fused local-motion route has no hot-pixel corrections: condition the movie")


def _raw_patch_plan(shape, dev, reference_strategy, patch_sidelength, pixel_spacing, b_factor, frequency_range):
    """(patch side, plan) of a patch estimator on a RawMovie, after the estimator's own argument rules; raises
    McorrUnsupported for every patch size but the wave-per-row kernel's -- before anything is launched."""
    _, h, w = shape
    p = int(patch_sidelength)
    _check_patch_args(reference_strategy, p, h, w)
    pl = planmod.get_xc_plan(p, p, pixel_spacing, b_factor, frequency_range, dev)
    if not _wave_rows_geometry(pl.geom):
        raise _lib.McorrUnsupported(f"no raw patch kernel for {p}-px patches (1024 only)")
    return p, pl


def _patch_spectra_raw(rm: "RawMovie", pl):
    """_patch_spectra for a RawMovie: the 1024-px patch row pass reads the raw bytes and the gain
    (mc_xc_rows_forward_dual_raw) and subtracts each job's frame mean + box mean."""
    lib = _lib.load()
    t, h, w = rm.shape
    dev = rm.raw.device
    g = pl.geom
    st = stream_ptr(dev)

    def spectra(off, ex, frames, expo_b=None, min_expo=None):
        if min_expo is None or min_expo < 1:
            raise _lib.McorrUnsupported("the raw patch kernel needs mask exponents >= 1")
        sub = rm.sub[torch.as_tensor(frames, device=dev)].contiguous()  # each job's frame mean + box mean
        dual = expo_b is not None

        def rows_pass(a, n, T1, T1b):
            check(lib.mc_xc_rows_forward_dual_raw(ptr(rm.raw), rm.kind, ptr(rm.gain), h * w, ptr(off[a:a + n]), w,
                                                  ptr(ex[a:a + n]), ptr(expo_b[a:a + n]) if dual else None,
                                                  ptr(pl.mask), ptr(sub[a:a + n]), ptr(rm.mean_rstd), ptr(T1),
                                                  ptr(T1b), ptr(pl.tw_row), n, g,
                                                  ptr(pl.chord) if USE_ROW_CHORDS else None, st),
                  "mc_xc_rows_forward_dual_raw")

        return _filtered_spectra(pl, dev, int(off.numel()), rows_pass, dual)

    return spectra


def patch_field_raw(rm: RawMovie, pixel_spacing, reference_frame, reference_strategy, b_factor, frequency_range,
                    patch_sidelength, sub_pixel_refinement, temporal_smoothing, smoothing_window_size,
                    outlier_rejection, outlier_threshold):
    """patch_field of the conditioned movie (condition_movie, then the central-box statistics) straight from a
    RawMovie: the 1024-px patch row pass reads the raw bytes and the gain (mc_xc_rows_forward_dual_raw) and
    subtracts each job's frame mean + box mean.  Raises McorrUnsupported for any shape that needs another kernel
    (patch sizes other than 1024, a hot-pixel threshold); there is no silent fall-back."""
    _local_raw_check(rm)
    dev = rm.raw.device
    p, pl = _raw_patch_plan(rm.shape, dev, reference_strategy, patch_sidelength, pixel_spacing, b_factor,
                            frequency_range)
    spectra = _patch_spectra_raw(rm, pl)
    return _patch_field_core(rm.shape, dev, pl, p, pixel_spacing, reference_frame, reference_strategy,
                             sub_pixel_refinement, temporal_smoothing, smoothing_window_size, None,
                             outlier_rejection, outlier_threshold, spectra)


def warp_field_raw(rm: RawMovie, lattices, pixel_spacing, want_frames=True, want_sum=False, out_sum=None,
                   accumulate=False):
    """``warp(img, lattices, ...)`` (deformation-field lattices) of the conditioned movie without materialising it
    (mc_warp_frames_raw).  Raises McorrUnsupported outside the raw kernel's shapes.  `out_sum` / `accumulate` as in
    warp_rigid_raw (mc_warp_frames_raw_accumulate)."""
    _local_raw_check(rm)
    t, h, w = rm.shape
    dev = rm.raw.device
    total = _sum_target(out_sum, want_sum, accumulate, h, w, dev)
    lib = _lib.load()
    _, _, GH, GW = lattices.shape
    frames = torch.empty((t, h, w), dtype=torch.float32, device=dev) if want_frames else None
    scratch = _field_scratch(lib, t, h, w, GH, GW, dev)
    entry = lib.mc_warp_frames_raw_accumulate if accumulate else lib.mc_warp_frames_raw
    check(entry(ptr(rm.raw), rm.kind, ptr(rm.gain), ptr(rm.mu), t, h, w, ptr(lattices.contiguous()), GH, GW,
                float(pixel_spacing), ptr(scratch), ptr(frames), ptr(total), stream_ptr(dev)), "mc_warp_frames_raw")
    return frames, total


def warp_dose_weighted_sum_raw(rm: RawMovie, lattices, pixel_spacing, rigid, dose_per_frame, pre_exposure, voltage,
                               want_plain):
    """warp_dose_weighted_sum of the conditioned movie straight from a RawMovie: each chunk of frames (the
    WORKSPACE_BYTES rule of _row_major_sums) is warped from the raw bytes of its frame window, transformed and
    weighted, then dropped -- neither the conditioned nor the corrected fp32 movie is held.
    `want_plain`: the plain sum too, from the same warp launches (the first chunk stores it, the others add to it:
    ((s_0 + s_1) + s_2) + ... in chunk order).  Returns (dose-weighted sum, plain sum or None).  Raises
    McorrUnsupported for shapes outside the row-major kernels, with POLYPHASE_FOURIER_SHIFT, and for whatever the
    raw warps refuse."""
    t, h, w = rm.shape
    if POLYPHASE_FOURIER_SHIFT or not _full_row_major_ok(h, w):
        raise _lib.McorrUnsupported(f"no streamed dose weighting from raw frames of {h} x {w}")
    if not rigid:
        _local_raw_check(rm)  # before anything is launched
    plain = torch.empty((h, w), dtype=torch.float32, device=rm.raw.device) if want_plain else None
    warp_raw = warp_rigid_raw if rigid else warp_field_raw

    def forward_rows(a, n, S):  # the chunk's warped frames are released on return, before the next chunk's warp
        kw = dict(want_frames=True, out_sum=plain, accumulate=want_plain and a > 0)
        _rows_forward(warp_raw(rm.window(a, n), lattices[a:a + n], pixel_spacing, **kw)[0], 0, n, S)

    dw, _ = _row_major_sums(rm.shape, rm.raw.device, forward_rows, pixel_spacing=pixel_spacing,
                            dose_per_frame=dose_per_frame, pre_exposure=pre_exposure, voltage=voltage)
    return dw, plain


def corrected_sums(src, lattices, pixel_spacing, rigid, dose_per_frame=None, pre_exposure=0.0, voltage=300.0,
                   want_plain=False, want_frames=False):
    """THE three ways to make the aligned sum of a movie through `lattices` -> (sum, plain sum or None, frames or
    None).  `src`: an fp32 / fp16 (t, h, w) stack on the device, or a RawMovie, whose warps read the raw bytes (and
    raise McorrUnsupported where a fused kernel is missing).  `rigid`: the separable rigid warp.
    * no `dose_per_frame`: the plain sum, from the warp itself;
    * a dose and `want_frames`: the frames are an output anyway, so they are warped and then weighted
      (dose_weighted_sum); `want_plain`: the plain sum too, from the same warp launch;
    * a dose alone: warped, transformed and weighted a chunk at a time (warp_dose_weighted_sum[_raw]); the plain sum
      alongside is built for a RawMovie only."""
    ps = float(pixel_spacing)
    raw = isinstance(src, RawMovie)
    if raw:
        warp_src = warp_rigid_raw if rigid else warp_field_raw
    else:
        warp_src = lambda *a, **kw: warp(*a, rigid=rigid, **kw)  # noqa: E731
    if dose_per_frame is None:
        frames, total = warp_src(src, lattices, ps, want_frames=want_frames, want_sum=True)
        return total, None, frames
    dose = (float(dose_per_frame), float(pre_exposure), float(voltage))
    if want_frames:
        frames, plain = warp_src(src, lattices, ps, want_frames=True, want_sum=want_plain)
        return dose_weighted_sum(frames, ps, *dose), plain, frames
    if raw:
        total, plain = warp_dose_weighted_sum_raw(src, lattices, ps, rigid, *dose, want_plain)
        return total, plain, None
    if want_plain:
        raise ValueError("the plain sum next to a streamed dose-weighted sum is built for a RawMovie only")
    return warp_dose_weighted_sum(src, lattices, ps, rigid, *dose), None, None


def _raw_rows_forward(rm, first, n, S):
    """_rows_forward for a RawMovie: the row transforms of frames first .. first+n-1 from the raw bytes of their
    frame window (mc_full_rows_forward_raw), then the window's hot pixels as sparse corrections of the spectra
    (mc_full_rows_hot_correct).  One sequence for every consumer of a raw movie's row-major spectra."""
    lib = _lib.load()
    _, h, w = rm.shape
    dev = rm.raw.device
    win, pitch, st = rm.window(first, n), S.shape[2], stream_ptr(dev)
    off = torch.arange(n, device=dev, dtype=torch.int64) * (h * w)
    check(lib.mc_full_rows_forward_raw(ptr(win.raw), win.kind, ptr(win.gain), ptr(win.mu), ptr(off), ptr(S),
                                       ptr(planmod.get_twiddles(w, dev)), n, h, w, pitch, st),
          "mc_full_rows_forward_raw")
    if win.n_hot:
        check(lib.mc_full_rows_hot_correct(ptr(win.hot_keys), ptr(win.hot_rv), win.n_hot, 0, n, h, w, ptr(S),
                                           pitch, st), "mc_full_rows_hot_correct")


def fast_shifts(grid_px):
    """The (t, 2) fp32 shifts (sy, sx) the Fourier-shift routes apply for a rigid (2, t, 1, 1) field in pixels: the
    field negated, as correct_motion_fast forms them (correct_motion.py:473-476).  One helper for the fused sums of
    fp32 frames and of raw movies, so both routes use the same shift tensor."""
    return (-grid_px.detach()[:, :, 0, 0].transpose(0, 1).to(torch.float32)).contiguous()


def fast_shift_sums(src, shifts, pixel_spacing=1.0, dose_per_frame=None, pre_exposure=0.0, voltage=300.0,
                    want_plain=False):
    """fourier_shift(frames, shifts) followed by its plain sum and / or dose_weighted_sum, without the shifted
    frames: both are linear, so each chunk of frames is transformed forward once and the column pass multiplies each
    frame's spectrum by its phase ramp and accumulates the plain and / or exposure-weighted sums (_row_major_sums);
    one inverse transform per sum at the end.  `src`: an fp32 (t, h, w) tensor, or a RawMovie, whose chunks are
    transformed from the raw bytes of their frame window (mc_full_rows_forward_raw, then the window's hot pixels,
    mc_full_rows_hot_correct) -- the same launches on the same samples otherwise.  Returns (dose-weighted sum or
    None, plain sum or None): the plain sum without a dose, or with `want_plain`.  Raises McorrUnsupported for
    shapes outside the row-major kernels and with POLYPHASE_FOURIER_SHIFT, before any launch."""
    raw = isinstance(src, RawMovie)
    t, h, w = src.shape
    if POLYPHASE_FOURIER_SHIFT or not _full_row_major_ok(h, w):
        raise _lib.McorrUnsupported(f"no fused Fourier-shift sums for frames of {h} x {w}")
    dev = src.raw.device if raw else src.device

    forward_rows = (lambda a, n, S: _raw_rows_forward(src, a, n, S)) if raw else (
        lambda a, n, S: _rows_forward(src, a, n, S))
    return _row_major_sums(src.shape, dev, forward_rows, shifts.to(dev, torch.float32).contiguous(), pixel_spacing,
                           dose_per_frame, pre_exposure, voltage, want_plain=want_plain or dose_per_frame is None)


FOURIER_CROP_SIZES = ("heights 512, 1024, 2048, 4096 and 8184 and widths 128, 256, ..., 8192 and 11520 "
                      "(any combination)")


def fourier_crop_supported(h, w):
    """Frames mc_full_cols_crop bins by 2: (h, w) and (h/2, w/2) both sizes of the row-major transforms."""
    return ((_pow2(h) and 512 <= h <= 4096) or h == 8184) and ((_pow2(w) and 128 <= w <= 8192) or w == 11520)


def fourier_crop(src):
    """Fourier cropping by 2 per axis: per frame irfft2 of the rows -h/4 <= ky < h/4 and columns kx <= w/4 of
    rfft2(frame), at (h/2, w/2), the frame's sum kept (scale 1 / ((h/2)(w/2))).  `src`: an fp32 (t, h, w) tensor, or
    a RawMovie, whose chunks are transformed from the raw bytes (_raw_rows_forward: no fp32 movie).  Per chunk of
    frames (the WORKSPACE_BYTES rule over the spectrum and its cropped copy): rows forward at (h, w) ->
    mc_full_cols_crop -> rows inverse at (h/2, w/2) straight into the (t, h/2, w/2) fp32 result.  Raises
    McorrUnsupported for other shapes, before any launch."""
    raw = isinstance(src, RawMovie)
    t, h, w = src.shape
    if not fourier_crop_supported(h, w):
        raise _lib.McorrUnsupported(f"no Fourier crop for frames of {h} x {w}: it takes {FOURIER_CROP_SIZES}")
    lib = _lib.load()
    dev = src.raw.device if raw else src.device
    h2, w2 = h // 2, w // 2
    pitch, pitch2 = lib.mc_full_spectrum_pitch(w), lib.mc_full_spectrum_pitch(w2)
    tw_col, tw_row2 = planmod.get_twiddles(h, dev), planmod.get_twiddles(w2, dev)
    out = torch.empty((t, h2, w2), dtype=torch.float32, device=dev)
    chunk, spans = _chunks(t, (h * pitch + h2 * pitch2) * 8)
    S = torch.empty((chunk, h, pitch, 2), dtype=torch.float32, device=dev)
    S2 = torch.empty((chunk, h2, pitch2, 2), dtype=torch.float32, device=dev)
    st = stream_ptr(dev)
    for a, n in spans:
        if raw:
            _raw_rows_forward(src, a, n, S)
        else:
            _rows_forward(src, a, n, S)
        check(lib.mc_full_cols_crop(ptr(S), ptr(S2), ptr(tw_col), n, h, w, pitch, pitch2, st), "mc_full_cols_crop")
        off = torch.arange(a, a + n, device=dev, dtype=torch.int64) * (h2 * w2)
        check(lib.mc_full_rows_inverse(ptr(S2), ptr(out), ptr(off), w2, ptr(tw_row2), n, h2, w2, pitch2, st),
              "mc_full_rows_inverse")
    return out


_HOT_NONE = (1 << 63) - 1


def _warp_hot_correct(lib, rm, scratch, frames, total, st):
    """Add each hot pixel's delta, times the weight with which mc_warp_rigid_raw read it, into the outputs whose
    taps reach it.  Records are summed per output element in a fixed order (stable sorts, one writer each):
    frames and sum are reproducible bit for bit."""
    t, h, w = rm.shape
    m = rm.n_hot * 49
    dev = rm.raw.device
    rec_key = torch.empty(m, dtype=torch.int64, device=dev)
    rec_val = torch.empty(m, dtype=torch.float32, device=dev)
    check(lib.mc_warp_rigid_hot_taps(ptr(rm.hot_keys), ptr(rm.hot_rv), rm.n_hot, t, h, w, ptr(scratch),
                                     ptr(rec_key), ptr(rec_val), st), "mc_warp_rigid_hot_taps")
    if frames is not None:
        k, order = torch.sort(rec_key, stable=True)
        check(lib.mc_hot_scatter_add(ptr(k), ptr(rec_val[order].contiguous()), m, t * h * w, ptr(frames), st),
              "mc_hot_scatter_add")
    if total is not None:
        pk = torch.where(rec_key == _HOT_NONE, rec_key, rec_key % (h * w))
        k, order = torch.sort(pk, stable=True)
        check(lib.mc_hot_scatter_add(ptr(k), ptr(rec_val[order].contiguous()), m, h * w, ptr(total), st),
              "mc_hot_scatter_add")


def condition_movie(raw, gain=None, mean_zero=True, hot_pixel_threshold=None, return_hot_counts=False):
    """raw (t,h,w) u8 / i16 / f16 / f32 on the GPU -> fp32 frames: x * gain, minus the frame's
    own mean (examples/ttMotion.py:90-121, 174-199), in two passes over the raw bytes.  With
    `hot_pixel_threshold` (the example uses 10.0) the hot-pixel step of examples/ttMotion.py:127-172
    runs in between: the example's detection, a deterministic replacement (mc_condition_movie_hot)."""
    lib = _lib.load()
    if raw.dtype not in _RAW_KINDS:
        raise TypeError(f"unsupported raw frame type {raw.dtype}; use uint8, int16, float16 or float32")
    t, h, w = raw.shape
    dev = raw.device
    raw = raw.contiguous()
    if gain is not None:
        if tuple(gain.shape) != (h, w):
            raise ValueError(f"gain reference has shape {tuple(gain.shape)}, frames are {(h, w)}")
        gain = gain.to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty((t, h, w), dtype=torch.float32, device=dev)
    if hot_pixel_threshold is not None:
        stats = torch.empty(3 * t, dtype=torch.float64, device=dev)
        counts = torch.empty(t, dtype=torch.int32, device=dev)
        check(lib.mc_condition_movie_hot(ptr(raw), _RAW_KINDS[raw.dtype], ptr(gain), t, h, w,
                                         1 if mean_zero else 0, float(hot_pixel_threshold), ptr(stats),
                                         ptr(counts), ptr(out), stream_ptr(dev)), "mc_condition_movie_hot")
        return (out, counts) if return_hot_counts else out
    sums = torch.empty(t, dtype=torch.float64, device=dev) if mean_zero else None
    check(lib.mc_condition_movie(ptr(raw), _RAW_KINDS[raw.dtype], ptr(gain), t, h * w, 1 if mean_zero else 0,
                                 ptr(sums), ptr(out), stream_ptr(dev)), "mc_condition_movie")
    return (out, torch.zeros(t, dtype=torch.int32, device=dev)) if return_hot_counts else out


GROUP_WINDOW_MAX = {torch.uint8: 128, torch.int16: 32768}  # frames of a window whose sum stays exact (raw_group.hip)


def check_group(group, t, dtype):
    """`group` as an int >= 1 (bools refused) whose window of min(group, t) frames the kernel sums exactly;
    ValueError otherwise (before anything is launched)."""
    try:
        g = None if isinstance(group, bool) else operator.index(group)
    except TypeError:
        g = None
    if g is None or g < 1:
        raise ValueError(f"group must be an int >= 1, got {group!r}")
    group = g
    if min(group, t) > GROUP_WINDOW_MAX[dtype]:
        raise ValueError(f"group={group}: a window of {min(group, t)} {dtype} frames is more than the "
                         f"{GROUP_WINDOW_MAX[dtype]} whose sum is exact")
    return group


def group_frames_raw(raw, group):
    """raw (t,h,w) u8 / i16 on the GPU -> the int16 (t,h,w) movie of rolling frame-group sums: frame i is the sum of
    the frames max(0, i - (group - 1) // 2) .. min(t - 1, i + group // 2) (mc_raw_group_frames).  Exact integers;
    an i16 window sum outside int16 raises ValueError (the flag's read is the one device-to-host copy).  Nothing
    frame-sized is allocated besides the output."""
    lib = _lib.load()
    t, h, w = raw.shape
    dev = raw.device
    group = check_group(group, t, raw.dtype)
    raw = raw.contiguous()
    out = torch.empty((t, h, w), dtype=torch.int16, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    # (a reach of t frames covers the movie from any frame: 2 t stands for every larger group)
    check(lib.mc_raw_group_frames(ptr(raw), _RAW_KINDS[raw.dtype], t, h, w, min(group, 2 * t), ptr(out), ptr(flag),
                                  stream_ptr(dev)), "mc_raw_group_frames")
    if raw.dtype == torch.int16 and int(flag.item()):
        raise ValueError(f"group={group}: a sum of {min(group, t)} frames of this int16 movie leaves the int16 range "
                         "[-32768, 32767]; use a smaller group")
    return out


def sum_frames(frames):
    lib = _lib.load()
    t, h, w = frames.shape
    total = torch.empty((h, w), dtype=torch.float32, device=frames.device)
    check(lib.mc_sum_frames(ptr(frames), t, h * w, ptr(total), stream_ptr(frames.device)),
          "mc_sum_frames")
    return total
