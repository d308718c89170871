"""The cross-correlation estimate: the K1 / K2 / K3 loops, the spectra of whole frames and the global shifts."""

from __future__ import annotations

import ctypes as C

import torch

from .. import _lib, engine as E, plan as planmod
from .._lib import check, ptr, stream_ptr


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
    """The geometry of the wave-per-row patch kernels (mc_xc_rows_forward_dual_*): rows of 1024 samples.
    A shortcut: the authority is wave512_shape (csrc/xc_rows_fwd.hip)."""
    return g.W == 1024 and g.nkx <= 128 and g.ny % 8 == 0


def _wave512_ok(g, job_expo, use_mask, min_expo):
    """Patch rows of 1024 samples can take the wave-per-row K1 (mc_xc_rows_forward_dual_t):
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
    chunk, spans = E._chunks(njobs, g.nkx * g.ny * 8 * (2 if dual else 1))
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
            check(lib.mc_xc_rows_forward_dual_t(ptr(src), E.storage_of(src), ptr(off), row_stride, ptr(expo),
                                                ptr(expo_b), ptr(pl.mask), ptr(stats), ptr(T1), ptr(T1b),
                                                ptr(pl.tw_row), n, g,
                                                ptr(pl.chord) if E.USE_ROW_CHORDS else None, st),
                  "mc_xc_rows_forward_dual_t")
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
    chunk, spans = E._chunks(npairs, g.nkx * g.H * 8)
    T2 = torch.empty((chunk, g.nkx, g.H, 2), dtype=torch.float32, device=dev)
    ngrp = g.H // g.RG
    pv = torch.empty(chunk * ngrp + chunk * g.H, dtype=torch.float32, device=dev)
    pi = torch.empty(chunk * ngrp + chunk + 1, dtype=torch.int32, device=dev)
    st = stream_ptr(dev)
    scale = 1.0 / (g.H * g.W)
    # near-window search (+ the 3x3 neighbourhood of the peak when asked): the full map (T2) is
    # a device-side fallback that normally never runs (mc_xc_correlate_argmax)
    fused = E.FUSED_SEARCH and planmod.native_rows(g) and planmod.native_height(g.H) and g.H >= 1024
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
        mhat = _forward_spectra(ones, off, g.W, None, pl, None, use_filter=False)[0].contiguous()
        torch.cuda.current_stream(dev).synchronize()  # cached on the plan, read from any stream: as plan.get_xc_plan
        pl.mhat = mhat
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
    job_off = E._cached(("frame_off", str(dev), t, h, w),
                      lambda: torch.arange(t, device=dev, dtype=torch.int64) * (h * w))
    fused = (planmod.native_rows(g) and planmod.native_height(g.H) and hl >= g.y0 and hu <= g.y0 + g.ny and wl >= g.x0
             and wu <= g.x1 and wl % 2 == 0 and wu % 2 == 0 and hu > hl and wu > wl)
    # fp16 frames are read as they are by the wave-per-row K1 (4096 columns); any other shape widens once
    half_ok = (img.dtype == torch.float16 and fused and w == 4096 and g.nkx <= 512 and g.ny % 8 == 0
               and wl % 256 == 0 and wu % 256 == 0 and img.data_ptr() % 16 == 0)
    if img.dtype != torch.float32 and not half_ok:
        img = img.float()
    if not fused:
        return _forward_spectra(img, job_off, w, None, pl, E.central_box_stats(img))
    st = stream_ptr(dev)
    mhat = mask_spectrum(pl, dev)
    # provisional mean m0 keeps the linear fix-up free of cancellation; any value near the
    # true mean does, so one row of frame 0's box is enough (one small workgroup)
    acc = torch.empty(128, dtype=torch.float64, device=dev)  # 64 x {sum, sumsq}
    m0 = torch.empty(3, dtype=torch.float32, device=dev)
    check(lib.mc_xc_provisional_mean_t(C.c_void_p(img.data_ptr() + img.element_size() * (hl * w + wl)),
                                       E.storage_of(img), wu - wl, ptr(m0), st), "mc_xc_provisional_mean_t")
    fix = torch.empty(2, dtype=torch.float32, device=dev)
    out3 = torch.empty(3, dtype=torch.float32, device=dev)
    T1 = torch.empty((t, g.nkx, g.ny, 2), dtype=torch.float32, device=dev)
    S = torch.empty((t, g.nkx, g.nky, 2), dtype=torch.float32, device=dev)
    try:
        check(lib.mc_xc_rows_forward_stats_t(ptr(img), E.storage_of(img), ptr(job_off), w, ptr(pl.mask), ptr(m0),
                                             ptr(T1), ptr(pl.tw_row), t, g, hl, hu, wl, wu, ptr(acc), ptr(fix),
                                             ptr(out3), ptr(_box_chords(pl, hl, hu, wl, wu)), st),
              "mc_xc_rows_forward_stats_t")
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


def _box_chords(pl, hl, hu, wl, wu):
    """The plan's per-row chord table if the statistics box lies inside the chords (it does for
    the reference's circular mask: the box corner is at 0.35 n from the centre, the soft edge ends
    at 0.375 n), else None: K1 then clamps to the support box only."""
    if pl.chord is None or not E.USE_ROW_CHORDS:
        return None
    key = ("chord_ok", id(pl), hl, hu, wl, wu)

    def build():
        c = pl.chord[hl:hu]
        return bool((c[:, 0] <= wl).all()) and bool((c[:, 1] + 4 >= wu).all())

    return pl.chord if E._cached(key, build) else None


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
    cur_idx, ref_idx = E._cached(
        ("global_pairs", str(dev), t, ref, skip),
        lambda: (E._i32(cur, dev), E._i32([ref] * len(cur), dev)))
    # pair p = frame cur[p]: its shift goes to row cur[p] of the (t, 2) table; the reference
    # frame's row is written by nobody and stays exactly zero
    _, shifts, _ = _peaks(S, cur_idx, S, ref_idx, pl, want_nbhd=False, shift_rows=cur_idx, n_shift_rows=t)
    return shifts
