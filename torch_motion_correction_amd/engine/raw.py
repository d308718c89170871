"""RawMovie and every route that reads a raw u8 / i16 movie without an fp32 copy; the three ways to an aligned sum."""

from __future__ import annotations

import math

import torch

from .. import _lib, engine as E, plan as planmod
from .._lib import check, ptr, stream_ptr


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


def _on_boundary(x, nbytes=16):
    """`x` where it starts on an `nbytes` boundary (or is None), else one copy of it that does: the staging rule of
    every tensor the raw kernels read with vector loads."""
    return x if x is None or x.data_ptr() % nbytes == 0 else x.clone()


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
    device-to-host copy; more hot pixels than hot_list_capacity() raise McorrUnsupported.

    The raw kernels read `raw` and `gain` in 16-byte units: a movie or a gain that starts off a 16-byte boundary
    (a view out of a larger buffer) is restaged here, with one copy; neither is ever written."""

    def __init__(self, raw, gain, mean_zero=True, hot_pixel_threshold=None):
        thr = check_hot_pixel_threshold(hot_pixel_threshold)
        lib = _lib.load()
        if raw.dtype not in (torch.uint8, torch.int16):
            raise TypeError(f"the fused raw path reads uint8 or int16 frames, got {raw.dtype}")
        t, h, w = raw.shape
        dev = raw.device
        self.raw = _on_boundary(raw.contiguous())
        self.gain = (torch.ones((h, w), dtype=torch.float32, device=dev) if gain is None
                     else _on_boundary(gain.detach().to(device=dev, dtype=torch.float32).contiguous()))
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
        cap = E.hot_list_capacity(t, h, w)
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

    def staged(self):
        """This movie where `raw` and `gain` start on a 16-byte boundary and the {r, v} pairs of `hot_rv` on an
        8-byte one (every movie the constructor built, and every window of one); else a shallow copy of it with one
        restaging copy of each of the three that does not (a movie whose tensors were since replaced by views out
        of larger buffers).  The first line of every route that hands them to a raw kernel: those refuse
        (MC_ERR_UNSUPPORTED) what is off its boundary."""
        if self.raw.data_ptr() % 16 == 0 and self.gain.data_ptr() % 16 == 0 and \
                (self.hot_rv is None or self.hot_rv.data_ptr() % 8 == 0):
            return self
        rm = object.__new__(E.RawMovie)
        rm.__dict__.update(self.__dict__)
        rm.raw, rm.gain, rm.hot_rv = _on_boundary(self.raw), _on_boundary(self.gain), _on_boundary(self.hot_rv, 8)
        return rm

    def window(self, a, n):
        """Frames [a, a+n) as a RawMovie of their own, without a copy of the movie: views of raw / mu / sub /
        stats / hot_counts, the same gain and mean_rstd, and the hot pixels of those frames -- the slice of the
        sorted `hot_keys` in [a*h*w, (a+n)*h*w), rebased to the window's first frame.  The warps and their hot-pixel
        corrections (_warp_hot_correct) then work per window unchanged.  (Views of the staged() movie: of this one
        unless its tensors were replaced by ones off their boundary.)"""
        t, h, w = self.shape
        if not (0 <= a and n >= 1 and a + n <= t):
            raise ValueError(f"frame window [{a}, {a + n}) outside a movie of {t} frames")
        hw = h * w
        src = self.staged()
        win = object.__new__(E.RawMovie)
        win.raw = src.raw[a:a + n]
        # the raw kernels read 16-byte units from the first frame's first byte (h*w % 64 == 0 on every
        # row-major shape, so every window of those is aligned)
        assert win.raw.data_ptr() % 16 == 0, "frame window not 16-byte aligned"
        win.gain, win.kind, win.shape = src.gain, src.kind, (n, h, w)
        win.hot_pixel_threshold = src.hot_pixel_threshold
        win.stats, win.mu, win.sub, win.mean_rstd = src.stats[a:a + n], src.mu[a:a + n], src.sub[a:a + n], src.mean_rstd
        win.n_hot = 0
        win.hot_keys = win.hot_rv = win.hot_counts = None
        if src.hot_counts is not None:
            win.hot_counts = src.hot_counts[a:a + n]
        if src.n_hot:
            if getattr(self, "_frame_starts", None) is None:  # one device-to-host copy per movie
                bounds = torch.arange(t + 1, device=self.raw.device, dtype=torch.int64) * hw
                self._frame_starts = torch.searchsorted(self.hot_keys, bounds).tolist()
            lo, hi = self._frame_starts[a], self._frame_starts[a + n]
            win.n_hot = hi - lo
            win.hot_keys = src.hot_keys[lo:hi] - a * hw
            win.hot_rv = src.hot_rv[lo:hi]
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


def global_shifts_raw(rm: E.RawMovie, reference_frame, pixel_spacing, b_factor, frequency_range, after_k1=None):
    """global_shifts for a RawMovie: K1 reads the raw bytes (mc_xc_rows_forward_raw / mc_xcg_rows_forward_raw), the
    statistics are known beforehand, so the plain column pass follows.  Raises McorrUnsupported for shapes
    without a fused kernel.  `after_k1()`, if given, is called once the last chunk's K1 (and hot-pixel fix-up)
    has been enqueued."""
    S, pl = _global_spectra_raw(rm, reference_frame, pixel_spacing, b_factor, frequency_range, after_k1)
    return E._shifts_from_spectra(S, rm.shape[0], reference_frame, pl)


def _global_spectra_raw(rm, reference_frame, pixel_spacing, b_factor, frequency_range, after_k1=None):
    """The filtered pruned spectra of global_shifts_raw and their plan -> (S (t, nkx, nky, 2), plan)."""
    lib = _lib.load()
    rm = rm.staged()
    t, h, w = rm.shape
    dev = rm.raw.device
    _lib.normalize_frame_index(reference_frame, t)  # IndexError before any launch, as the fp32 path
    pl = planmod.get_xc_plan(h, w, pixel_spacing, b_factor, frequency_range, dev)
    g = pl.geom
    if not raw_fused_supported(rm.raw, pl):
        raise _lib.McorrUnsupported("no fused raw kernel for this frame shape")
    st = stream_ptr(dev)
    job_off = E._cached(("frame_off", str(dev), t, h, w),
                      lambda: torch.arange(t, device=dev, dtype=torch.int64) * (h * w))
    chord = ptr(pl.chord) if (pl.chord is not None and E.USE_ROW_CHORDS) else None

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

    return E._filtered_spectra(pl, dev, t, rows_pass), pl


def global_shifts_raw_refined(rm: E.RawMovie, reference_frame, pixel_spacing, b_factor, frequency_range, start=None,
                              max_iterations=10, threshold=0.01):
    """global_shifts_raw followed by refine_shifts_from_spectra on the same spectra -> ((t, 2) px, history).  Raises
    McorrUnsupported for shapes without a fused raw kernel, as global_shifts_raw."""
    S, pl = _global_spectra_raw(rm, reference_frame, pixel_spacing, b_factor, frequency_range)
    return E.refine_shifts_from_spectra(S, rm.shape[0], reference_frame, pl, start, max_iterations, threshold)


def warp_rigid_raw(rm: E.RawMovie, lattices, pixel_spacing, want_frames=True, want_sum=False, tables=None,
                   out_sum=None, accumulate=False):
    """``warp(..., rigid=True)`` of the conditioned movie without materialising it (mc_warp_rigid_raw).
    `out_sum`: the (h, w) buffer the sum goes to (implies want_sum); with `accumulate` the sum is added to what it
    holds (mc_warp_rigid_raw_accumulate) -- the hot-pixel corrections of these frames too."""
    rm = rm.staged()
    t, h, w = rm.shape
    dev = rm.raw.device
    total = E._sum_target(out_sum, want_sum, accumulate, h, w, dev)
    lib = _lib.load()
    frames = torch.empty((t, h, w), dtype=torch.float32, device=dev) if want_frames else None
    entry = lib.mc_warp_rigid_raw_accumulate if accumulate else lib.mc_warp_rigid_raw
    if tables is None:
        shifts_px = E.rigid_shifts_px(lattices, pixel_spacing)
        scratch = E._rigid_scratch(lib, t, h, w, dev)
        phase = 0
    else:
        shifts_px, scratch = tables
        phase = 2
    run = lambda: check(entry(ptr(rm.raw), rm.kind, ptr(rm.gain), ptr(rm.mu), t, h, w, ptr(shifts_px), ptr(scratch),
                              ptr(frames), ptr(total), phase, stream_ptr(dev)), "mc_warp_rigid_raw")
    if E.RIGID_KERNEL_HOOK is not None and phase == 2:
        E.RIGID_KERNEL_HOOK(run)
    else:
        run()
    if rm.n_hot:
        _warp_hot_correct(lib, rm, scratch, frames, total, stream_ptr(dev))
    return frames, total


def _local_raw_check(rm: E.RawMovie):
    if rm.hot_pixel_threshold is not None:
        raise _lib.McorrUnsupported("the fused local-motion route has no hot-pixel corrections: condition the movie")


def _raw_patch_plan(shape, dev, reference_strategy, patch_sidelength, pixel_spacing, b_factor, frequency_range):
    """(patch side, plan) of a patch estimator on a RawMovie, after the estimator's own argument rules; raises
    McorrUnsupported for every patch size but the wave-per-row kernel's -- before anything is launched."""
    _, h, w = shape
    p = int(patch_sidelength)
    E._check_patch_args(reference_strategy, p, h, w)
    pl = planmod.get_xc_plan(p, p, pixel_spacing, b_factor, frequency_range, dev)
    if not E._wave_rows_geometry(pl.geom):
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
                                                  ptr(pl.chord) if E.USE_ROW_CHORDS else None, st),
                  "mc_xc_rows_forward_dual_raw")

        return E._filtered_spectra(pl, dev, int(off.numel()), rows_pass, dual)

    return spectra


def patch_field_raw(rm: E.RawMovie, pixel_spacing, reference_frame, reference_strategy, b_factor, frequency_range,
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
    return E._patch_field_core(rm.shape, dev, pl, p, pixel_spacing, reference_frame, reference_strategy,
                             sub_pixel_refinement, temporal_smoothing, smoothing_window_size, None,
                             outlier_rejection, outlier_threshold, spectra)


def warp_field_raw(rm: E.RawMovie, lattices, pixel_spacing, want_frames=True, want_sum=False, out_sum=None,
                   accumulate=False):
    """``warp(img, lattices, ...)`` (deformation-field lattices) of the conditioned movie without materialising it
    (mc_warp_frames_raw).  Raises McorrUnsupported outside the raw kernel's shapes.  `out_sum` / `accumulate` as in
    warp_rigid_raw (mc_warp_frames_raw_accumulate)."""
    _local_raw_check(rm)
    rm = rm.staged()
    t, h, w = rm.shape
    dev = rm.raw.device
    total = E._sum_target(out_sum, want_sum, accumulate, h, w, dev)
    lib = _lib.load()
    _, _, GH, GW = lattices.shape
    frames = torch.empty((t, h, w), dtype=torch.float32, device=dev) if want_frames else None
    scratch = E._field_scratch(lib, t, h, w, GH, GW, dev)
    entry = lib.mc_warp_frames_raw_accumulate if accumulate else lib.mc_warp_frames_raw
    check(entry(ptr(rm.raw), rm.kind, ptr(rm.gain), ptr(rm.mu), t, h, w, ptr(lattices.contiguous()), GH, GW,
                float(pixel_spacing), ptr(scratch), ptr(frames), ptr(total), stream_ptr(dev)), "mc_warp_frames_raw")
    return frames, total


def warp_dose_weighted_sum_raw(rm: E.RawMovie, lattices, pixel_spacing, rigid, dose_per_frame, pre_exposure, voltage,
                               want_plain):
    """warp_dose_weighted_sum of the conditioned movie straight from a RawMovie: each chunk of frames (the
    WORKSPACE_BYTES rule of _row_major_sums) is warped from the raw bytes of its frame window, transformed and
    weighted, then dropped -- neither the conditioned nor the corrected fp32 movie is held.
    `want_plain`: the plain sum too, from the same warp launches (the first chunk stores it, the others add to it:
    ((s_0 + s_1) + s_2) + ... in chunk order).  Returns (dose-weighted sum, plain sum or None).  Raises
    McorrUnsupported for shapes outside the row-major kernels, with POLYPHASE_FOURIER_SHIFT, and for whatever the
    raw warps refuse."""
    t, h, w = rm.shape
    if E.POLYPHASE_FOURIER_SHIFT or not E._full_row_major_ok(h, w):
        raise _lib.McorrUnsupported(f"no streamed dose weighting from raw frames of {h} x {w}")
    if not rigid:
        _local_raw_check(rm)  # before anything is launched
    plain = torch.empty((h, w), dtype=torch.float32, device=rm.raw.device) if want_plain else None
    warp_raw = warp_rigid_raw if rigid else warp_field_raw

    def forward_rows(a, n, S):  # the chunk's warped frames are released on return, before the next chunk's warp
        kw = dict(want_frames=True, out_sum=plain, accumulate=want_plain and a > 0)
        E._rows_forward(warp_raw(rm.window(a, n), lattices[a:a + n], pixel_spacing, **kw)[0], 0, n, S)

    dw, _ = E._row_major_sums(rm.shape, rm.raw.device, forward_rows, pixel_spacing=pixel_spacing,
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
    raw = isinstance(src, E.RawMovie)
    if raw:
        warp_src = warp_rigid_raw if rigid else warp_field_raw
    else:
        warp_src = lambda *a, **kw: E.warp(*a, rigid=rigid, **kw)  # noqa: E731
    if dose_per_frame is None:
        frames, total = warp_src(src, lattices, ps, want_frames=want_frames, want_sum=True)
        return total, None, frames
    dose = (float(dose_per_frame), float(pre_exposure), float(voltage))
    if want_frames:
        frames, plain = warp_src(src, lattices, ps, want_frames=True, want_sum=want_plain)
        return E.dose_weighted_sum(frames, ps, *dose), plain, frames
    if raw:
        total, plain = warp_dose_weighted_sum_raw(src, lattices, ps, rigid, *dose, want_plain)
        return total, plain, None
    if want_plain:
        raise ValueError("the plain sum next to a streamed dose-weighted sum is built for a RawMovie only")
    return E.warp_dose_weighted_sum(src, lattices, ps, rigid, *dose), None, None


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
