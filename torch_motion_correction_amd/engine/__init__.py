"""Device-side pipelines on top of libmcorr (all tensors already on the GPU).

These functions only allocate buffers (torch caching allocator), build small index
tables and enqueue libmcorr kernels on the current stream; they never synchronise (one exception:
a RawMovie with a hot-pixel threshold reads the length of its hot-pixel list back).

ONE namespace, a module per kernel family.  This package is the only home of the test switches, the benchmark hook,
the limits and the small helpers every family uses; below them it imports the family modules and re-exports every
name of theirs.  A family module reaches a switch, the hook, a helper and any function of ANOTHER family as
``E.NAME`` (``from .. import engine as E``) inside its functions, i.e. at call time: what a caller or a test assigns
or replaces here is what the engine runs.
"""

from __future__ import annotations

# (C, math, operator, lattice, spline: names of this namespace since it was one module; a family imports its own)
import ctypes as C  # noqa: F401
import math  # noqa: F401
import operator  # noqa: F401
import os

import numpy as np
import torch

from .. import _lib, lattice, plan as planmod, spline  # noqa: F401
from .._lib import check, ptr, stream_ptr

# ------------------------------------------------------------------ switches, hook, limits


def _os_env_flag(name, default):
    v = os.environ.get(name)
    return default if v is None else v not in ("0", "false", "no")


WORKSPACE_BYTES = 2 << 30  # soft cap for one transposed intermediate (T1 / T2)
FUSED_SEARCH = True  # near-window arg-max (mc_xc_correlate_argmax); False: full T2 + separate kernels
USE_ROW_CHORDS = _os_env_flag("MC_ROW_CHORDS", True)
FULL_ROW_MAJOR = True  # tests: False forces the pruned engine's transposed layout on power-of-two frames
DOSE_COLUMN_MAJOR = True  # tests / A-B: False feeds the exposure-weighted pass from the row-major spectra
POLYPHASE_FOURIER_SHIFT = False  # tests: force the x-polyphase form on frames that do not need it

RIGID_KERNEL_HOOK = None  # callable(fn) -> calls fn(); set by bench.py to time warp_rigid_dma alone

REFINE_MAX_FRAMES = 512  # mc_xc_aligned_refs / mc_xc_refine_update
FOURIER_CROP_SIZES = ("heights 512, 1024, 2048, 4096 and 8184 and widths 128, 256, ..., 8192 and 11520 "
                      "(any combination)")
FOURIER_CROP_TO_SIZES = ("heights 512 -> 384, 4096 -> 3072, 4092 -> 2046, 8184 -> 5456 and 8184 -> 2728 with widths "
                         "64, 128, ..., 8192, 5760 and 11520 -> any of those or 2880, 3072, 3840 and 7680 that is no "
                         "wider (any combination), and the halving of " + FOURIER_CROP_SIZES)
GROUP_WINDOW_MAX = {torch.uint8: 128, torch.int16: 32768}  # frames of a window whose sum stays exact (raw_group.hip)


# ------------------------------------------------------------------ shared helpers


_CONST: dict = {}  # any stream may read an entry: _cached synchronises the stream that built it, once per key


def _cached(key, build):
    """Small device-resident index/tap tables, built once per (shape, device).  Some builders copy from host memory
    (blocking), some run a device kernel (torch.arange on the device) on the current stream: the building stream is
    synchronised (_sync_built: the current stream of the TABLES' device, which need not be the current device)
    before the entry is stored, because every later call reads it from whichever stream is current then, with no
    ordering against this one."""
    v = _CONST.get(key)
    if v is None:
        if len(_CONST) > 512:
            _CONST.clear()
        v = build()
        _sync_built(v)
        _CONST[key] = v
    return v


def _sync_built(v):
    """Synchronise the current stream of every device a freshly built table (a tensor, or tuples of them) lives on:
    the stream its builder ran on."""
    if isinstance(v, torch.Tensor):
        if v.is_cuda:
            torch.cuda.current_stream(v.device).synchronize()
    elif isinstance(v, (tuple, list)):
        for x in v:
            _sync_built(x)


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
                                     stream_ptr(img.device)), "mc_central_box_stats_t")
    return out3


def normalize(img: torch.Tensor, stats: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    out = torch.empty_like(img)
    check(lib.mc_normalize(ptr(img), ptr(out), img.numel(), ptr(stats), stream_ptr(img.device)),
          "mc_normalize")
    return out


# ------------------------------------------------------------------ the kernel families (after everything above)

from .xc import (  # noqa: E402
    _box_chords, _filtered_spectra, _forward_spectra, _global_spectra, _k1, _k2, _peaks, _shifts_from_spectra,
    _wave512_ok, _wave_rows_geometry, global_shifts, mask_spectrum)
from .refine import (  # noqa: E402
    _kept_frequencies, _local_shifts_refined, check_refine_args, global_shifts_refined, local_shifts_raw_refined,
    local_shifts_refined, patch_origins, refine_patch_shifts, refine_shifts_from_spectra, refine_under_px,
    refine_window_offsets, start_field_px)
from .patches import _check_patch_args, _patch_field_core, _patch_spectra, patch_field  # noqa: E402
from .warps import (  # noqa: E402
    _field_scratch, _rigid_scratch, _sum_target, frame_lattices, pixel_shifts, pixel_shifts_at, rigid_shifts_px,
    rigid_tables, rigid_tables_from_shifts, spline_lattice, spline_points, warp)
from .fourier import (  # noqa: E402
    _dose_weighted_sum_polyphase, _fourier_shift_polyphase, _fourier_shift_row_major, _full_row_major_ok,
    _full_spectra_chunks, _inverse_frames, _polyphase_geometry, _row_major_sums, _rows_forward, dose_weighted_sum,
    CROP_TO_HEIGHTS, CROP_TO_WIDTHS_IN, CROP_TO_WIDTHS_OUT, fast_shift_sums, fast_shifts, fourier_crop,
    fourier_crop_supported, fourier_crop_to, fourier_crop_to_shapes, fourier_crop_to_supported, fourier_shift,
    warp_dose_weighted_sum)
from .raw import (  # noqa: E402
    _HOT_NONE, _RAW_KINDS, RawMovie, _global_spectra_raw, _local_raw_check, _on_boundary, _patch_spectra_raw,
    _raw_patch_plan, _raw_rows_forward, _warp_hot_correct, check_hot_pixel_threshold, corrected_sums, global_shifts_raw,
    global_shifts_raw_refined, hot_list_capacity, patch_field_raw, raw_fused_supported, warp_dose_weighted_sum_raw,
    warp_field_raw, warp_rigid_raw)
from .condition import check_group, condition_movie, group_frames_raw, sum_frames  # noqa: E402
