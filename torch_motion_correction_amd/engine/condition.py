"""Conditioning of raw movies into fp32 frames, rolling frame-group sums, the plain frame sum."""

from __future__ import annotations

import operator

import torch

from .. import _lib, engine as E
from .._lib import check, ptr, stream_ptr


def condition_movie(raw, gain=None, mean_zero=True, hot_pixel_threshold=None, return_hot_counts=False):
    """raw (t,h,w) u8 / i16 / f16 / f32 on the GPU -> fp32 frames: x * gain, minus the frame's
    own mean (examples/ttMotion.py:90-121, 174-199), in two passes over the raw bytes.  With
    `hot_pixel_threshold` (the example uses 10.0) the hot-pixel step of examples/ttMotion.py:127-172
    runs in between: the example's detection, a deterministic replacement (mc_condition_movie_hot)."""
    lib = _lib.load()
    if raw.dtype not in E._RAW_KINDS:
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
        check(lib.mc_condition_movie_hot(ptr(raw), E._RAW_KINDS[raw.dtype], ptr(gain), t, h, w,
                                         1 if mean_zero else 0, float(hot_pixel_threshold), ptr(stats),
                                         ptr(counts), ptr(out), stream_ptr(dev)), "mc_condition_movie_hot")
        return (out, counts) if return_hot_counts else out
    sums = torch.empty(t, dtype=torch.float64, device=dev) if mean_zero else None
    check(lib.mc_condition_movie(ptr(raw), E._RAW_KINDS[raw.dtype], ptr(gain), t, h * w, 1 if mean_zero else 0,
                                 ptr(sums), ptr(out), stream_ptr(dev)), "mc_condition_movie")
    return (out, torch.zeros(t, dtype=torch.int32, device=dev)) if return_hot_counts else out


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
    if min(group, t) > E.GROUP_WINDOW_MAX[dtype]:
        raise ValueError(f"group={group}: a window of {min(group, t)} {dtype} frames is more than the "
                         f"{E.GROUP_WINDOW_MAX[dtype]} whose sum is exact")
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
    check(lib.mc_raw_group_frames(ptr(raw), E._RAW_KINDS[raw.dtype], t, h, w, min(group, 2 * t), ptr(out), ptr(flag),
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
