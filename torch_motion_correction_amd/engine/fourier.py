"""Full spectra: the Fourier shift, the dose-weighted and Fourier-shifted sums, Fourier cropping -- on the pruned
engine (also in polyphase form) and on the row-major kernels."""

from __future__ import annotations

import torch

from .. import _lib, engine as E, plan as planmod
from .._lib import check, ptr, stream_ptr


# ------------------------------------------------------------------ a19: Fourier shift


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
    chunk, spans = E._chunks(t, 2 * k * g.nkx * g.H * 8)
    T1 = torch.empty((k * chunk, g.nkx, g.ny, 2), dtype=torch.float32, device=dev)
    S = torch.empty((k * chunk, g.nkx, g.nky, 2), dtype=torch.float32, device=dev)
    st = stream_ptr(dev)
    for a, n in spans:
        if polyphase:
            src = torch.cat([img[a:a + n, :, 0::2], img[a:a + n, :, 1::2]], dim=0).contiguous()  # (2n, h, w/2)
            off = torch.arange(2 * n, device=dev, dtype=torch.int64) * (h * wj)
        else:
            src, off = img, torch.arange(a, a + n, device=dev, dtype=torch.int64) * (h * w)
        check(E._k1(lib, g, dev, src, off, wj, None, None, None, T1, tw_row, k * n, st), "xc rows forward")
        check(E._k2(lib, g, dev, T1, None, S, tw_col, k * n, st), "xc cols forward")
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


def _full_row_major_ok(h, w):
    """Frames the row-major full-spectrum kernels (csrc/full_fft.hip, full_sums.hip) take: power-of-two rows and
    columns, and the K3 detector's 5760 / 11520 columns and 4092 / 8184 rows (mixed radix)."""
    rows_ok = (E._pow2(w) and 64 <= w <= 8192) or w in (5760, 11520)
    cols_ok = (E._pow2(h) and 256 <= h <= 4096) or h in (4092, 8184)
    return E.FULL_ROW_MAJOR and rows_ok and cols_ok


def _fourier_shift_row_major(img, shifts):
    """fourier_shift on power-of-two frames: rows forward -> (columns forward, phase ramp, columns
    inverse) in one in-place kernel -> rows inverse, the spectrum row-major throughout.  A stack that starts off an
    8-byte boundary is restaged a chunk at a time (_rows_forward's rule); the output is a fresh buffer."""
    lib = _lib.load()
    t, h, w = img.shape
    dev = img.device
    pitch = lib.mc_full_spectrum_pitch(w)
    tw_row, tw_col = planmod.get_twiddles(w, dev), planmod.get_twiddles(h, dev)
    out = torch.empty_like(img)
    chunk, spans = E._chunks(t, h * pitch * 8)
    S = torch.empty((chunk, h, pitch, 2), dtype=torch.float32, device=dev)
    st = stream_ptr(dev)
    shifts = shifts.to(dev, torch.float32).contiguous()
    for a, n in spans:
        off = torch.arange(a, a + n, device=dev, dtype=torch.int64) * (h * w)
        E._rows_forward(img, a, n, S)
        check(lib.mc_full_cols_shift(ptr(S), ptr(shifts[a:a + n]), ptr(tw_col), 1.0 / (h * w), n, h, w, pitch, st),
              "mc_full_cols_shift")
        check(lib.mc_full_rows_inverse(ptr(S), ptr(out), ptr(off), w, ptr(tw_row), n, h, w, pitch, st),
              "mc_full_rows_inverse")
    return out


def _rows_forward(src, first, n, S):
    """mc_full_rows_forward of the fp32 frames first .. first+n-1 of `src` (t, h, w) into S (chunk, h, pitch, 2).
    The row pass reads its samples in pairs and refuses a pointer that is not 8-byte aligned: a stack that starts
    4 bytes off (a view into a larger buffer) is copied, these n frames at a time, into an aligned one."""
    lib = _lib.load()
    _, h, w = src.shape
    dev = src.device
    if src.data_ptr() % 8:
        src, first = src[first:first + n].clone(), 0
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
    colmajor = E.DOSE_COLUMN_MAJOR and h in (4096, 4092)
    chunk, spans = E._chunks(t, (2 if colmajor else 1) * per_frame)
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
    if E.POLYPHASE_FOURIER_SHIFT or not _full_row_major_ok(h, w):
        frames, _ = E.warp(img, lattices, pixel_spacing, want_frames=True, want_sum=False, rigid=rigid)
        return dose_weighted_sum(frames, pixel_spacing, dose_per_frame, pre_exposure, voltage)

    def forward_rows(a, n, S):  # the chunk's warped frames are released on return, before the next chunk's warp
        frames = E.warp(img[a:a + n], lattices[a:a + n], pixel_spacing, want_frames=True, want_sum=False,
                        rigid=rigid)[0]
        E._rows_forward(frames, 0, n, S)

    return _row_major_sums(img.shape, img.device, forward_rows, pixel_spacing=pixel_spacing,
                           dose_per_frame=dose_per_frame, pre_exposure=pre_exposure, voltage=voltage)[0]


def fourier_shift(img, shifts):
    """irfft2(rfft2(img) * exp(-2 pi i (fy sy + fx sx))) per frame; shifts (t,2) px
    (correct_motion.py:484-496)."""
    lib = _lib.load()
    t, h, w = img.shape
    dev = img.device
    if E.POLYPHASE_FOURIER_SHIFT:
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
    if E.POLYPHASE_FOURIER_SHIFT:
        return _dose_weighted_sum_polyphase(img, pixel_spacing, dose_per_frame, pre_exposure, voltage)
    if _full_row_major_ok(h, w):
        return _row_major_sums(img.shape, dev, lambda a, n, S: E._rows_forward(img, a, n, S),
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
    raw = isinstance(src, E.RawMovie)
    t, h, w = src.shape
    if E.POLYPHASE_FOURIER_SHIFT or not _full_row_major_ok(h, w):
        raise _lib.McorrUnsupported(f"no fused Fourier-shift sums for frames of {h} x {w}")
    dev = src.raw.device if raw else src.device

    forward_rows = (lambda a, n, S: E._raw_rows_forward(src, a, n, S)) if raw else (
        lambda a, n, S: E._rows_forward(src, a, n, S))
    return _row_major_sums(src.shape, dev, forward_rows, shifts.to(dev, torch.float32).contiguous(), pixel_spacing,
                           dose_per_frame, pre_exposure, voltage, want_plain=want_plain or dose_per_frame is None)


def fourier_crop_supported(h, w):
    """Frames mc_full_cols_crop bins by 2: (h, w) and (h/2, w/2) both sizes of the row-major transforms."""
    return ((E._pow2(h) and 512 <= h <= 4096) or h == 8184) and ((E._pow2(w) and 128 <= w <= 8192) or w == 11520)


def fourier_crop(src, out_shape=None):
    """Fourier cropping by 2 per axis: per frame irfft2 of the rows -h/4 <= ky < h/4 and columns kx <= w/4 of
    rfft2(frame), at (h/2, w/2), the frame's sum kept (scale 1 / ((h/2)(w/2))).  `src`: an fp32 (t, h, w) tensor, or
    a RawMovie, whose chunks are transformed from the raw bytes (_raw_rows_forward: no fp32 movie).  Per chunk of
    frames (the WORKSPACE_BYTES rule over the spectrum and its cropped copy): rows forward at (h, w) ->
    mc_full_cols_crop -> rows inverse at (h/2, w/2) straight into the (t, h/2, w/2) fp32 result.  Raises
    McorrUnsupported for other shapes, before any launch.

    `out_shape` (fourier_crop_to's, which has checked it; None: the halving above, as ever): the same loop to
    (h2, w2) -- the rows -h2/2 <= ky < h2/2 and columns kx <= w2/2, scale 1 / (h2 w2) -- with mc_full_cols_crop_to
    as the column pass, which reads the h2-point twiddle table besides the h-point one."""
    raw = isinstance(src, E.RawMovie)
    t, h, w = src.shape
    if out_shape is None and not fourier_crop_supported(h, w):
        raise _lib.McorrUnsupported(f"no Fourier crop for frames of {h} x {w}: it takes {E.FOURIER_CROP_SIZES}")
    lib = _lib.load()
    dev = src.raw.device if raw else src.device
    h2, w2 = (h // 2, w // 2) if out_shape is None else out_shape
    pitch, pitch2 = lib.mc_full_spectrum_pitch(w), lib.mc_full_spectrum_pitch(w2)
    tw_col, tw_row2 = planmod.get_twiddles(h, dev), planmod.get_twiddles(w2, dev)
    tw_col2 = None if out_shape is None else planmod.get_twiddles(h2, dev)
    out = torch.empty((t, h2, w2), dtype=torch.float32, device=dev)
    chunk, spans = E._chunks(t, (h * pitch + h2 * pitch2) * 8)
    S = torch.empty((chunk, h, pitch, 2), dtype=torch.float32, device=dev)
    S2 = torch.empty((chunk, h2, pitch2, 2), dtype=torch.float32, device=dev)
    st = stream_ptr(dev)
    for a, n in spans:
        if raw:
            E._raw_rows_forward(src, a, n, S)
        else:
            E._rows_forward(src, a, n, S)
        if out_shape is None:
            check(lib.mc_full_cols_crop(ptr(S), ptr(S2), ptr(tw_col), n, h, w, pitch, pitch2, st), "mc_full_cols_crop")
        else:
            check(lib.mc_full_cols_crop_to(ptr(S), ptr(S2), ptr(tw_col), ptr(tw_col2), n, h, w, h2, w2, pitch, pitch2,
                                           st), "mc_full_cols_crop_to")
        off = torch.arange(a, a + n, device=dev, dtype=torch.int64) * (h2 * w2)
        check(lib.mc_full_rows_inverse(ptr(S2), ptr(out), ptr(off), w2, ptr(tw_row2), n, h2, w2, pitch2, st),
              "mc_full_rows_inverse")
    return out


# (h -> h2) pairs of mc_full_cols_crop_to; the widths mc_full_rows_forward reads and mc_full_rows_inverse writes
CROP_TO_HEIGHTS = {512: (384,), 4096: (3072,), 4092: (2046,), 8184: (5456, 2728)}
CROP_TO_WIDTHS_IN = tuple(1 << p for p in range(6, 14)) + (5760, 11520)
CROP_TO_WIDTHS_OUT = tuple(sorted(CROP_TO_WIDTHS_IN + (2880, 3072, 3840, 7680)))


def fourier_crop_to_supported(h, w, h2, w2):
    """Frames fourier_crop_to brings from (h, w) to (h2, w2): a height pair of mc_full_cols_crop_to with any width
    pair (w a forward row length, w2 <= w an inverse one) -- the axes are independent -- or the halving of both axes
    fourier_crop takes."""
    if (h2, w2) == (h // 2, w // 2) and h % 2 == 0 and w % 2 == 0 and fourier_crop_supported(h, w):
        return True
    return h2 in CROP_TO_HEIGHTS.get(h, ()) and w in CROP_TO_WIDTHS_IN and w2 in CROP_TO_WIDTHS_OUT and w2 <= w


def fourier_crop_to_shapes(h, w):
    """Every (h2, w2) fourier_crop_to_supported(h, w, h2, w2) holds for, sorted."""
    found = {(h2, w2) for h2 in CROP_TO_HEIGHTS.get(h, ()) for w2 in CROP_TO_WIDTHS_OUT
             if fourier_crop_to_supported(h, w, h2, w2)}
    if fourier_crop_to_supported(h, w, h // 2, w // 2):
        found.add((h // 2, w // 2))
    return sorted(found)


def fourier_crop_to(src, out_shape):
    """Fourier cropping to `out_shape` = (h2, w2): per frame irfft2 of the rows -h2/2 <= ky < h2/2 (the new Nyquist
    row from the negative side) and columns kx <= w2/2 of rfft2(frame), at (h2, w2), the frame's sum kept (scale
    1 / (h2 w2)).  `src` as for fourier_crop, whose chunk loop runs it with mc_full_cols_crop_to as the column pass;
    the halving of a frame fourier_crop takes IS fourier_crop (the same launches, the same bits).  Raises
    McorrUnsupported for every other pair of shapes, before any launch."""
    t, h, w = src.shape
    h2, w2 = int(out_shape[0]), int(out_shape[1])
    if not fourier_crop_to_supported(h, w, h2, w2):
        raise _lib.McorrUnsupported(f"no Fourier crop from {h} x {w} to {h2} x {w2}: it takes {E.FOURIER_CROP_TO_SIZES}")
    if (h2, w2) == (h // 2, w // 2) and fourier_crop_supported(h, w):
        return E.fourier_crop(src)
    return E.fourier_crop(src, (h2, w2))
