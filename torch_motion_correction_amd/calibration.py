"""Gain-reference and defect-map estimation from a session's own raw u8 / i16 movies.

Every raw route of the package takes ``(raw movie, gain)``; the reference's example loads that gain from a file
(examples/ttMotion.py:40-121).  Where no current file exists, facilities estimate one from the movies themselves
(relion_estimate_gain, MotionCor2's gain tools): the per-pixel mean over many frames, ``gain = mean of the good
pixels / pixel mean``, and a list of dead, hot and stuck pixels from the same statistics.

  RawStatistics            per-pixel sum and sum of squares over all frames added, exact 64-bit integers, from one
                           read of the raw bytes (mc_raw_pixel_sums, csrc/raw_accumulate.hip); nothing frame-sized
                           is allocated
  estimate_defect_map      dead / hot / stuck pixels of the session (pixels wrong in EVERY movie, which the per-movie
                           ``hot_pixel_threshold`` step cannot see)
  estimate_gain_reference  the fp32 gain in the package's convention (gain multiplies raw), 0 at defects

The finalisation is a handful of (h, w) torch operations once per session, on the device the statistics live on.
All rules are integer or single float64 operations, so tests/calibration_reference.py restates them bit for bit.
"""

from __future__ import annotations

import torch

from ._lib import check, device_scope, load, ptr, require_gpu, stream_ptr

RAW_DTYPES = (torch.uint8, torch.int16)
# sumsq is exposed as int64: after n frames it is at most 255^2 n (u8) or 2^30 n (i16, all -32768), which passes
# 2^63 - 1 beyond these frame counts.  add() and merge() refuse the frames that would exceed them.
MAX_FRAMES = {torch.uint8: (2**63 - 1) // 255**2, torch.int16: (2**63 - 1) // 2**30}
EXACT_F64 = 2**53  # integers below it convert to float64 exactly


class RawStatistics:
    """Per-pixel ``sum`` and ``sumsq`` (int64, (h, w)) of every raw frame added so far.

    ``shape`` is the frame size (h, w).  ``device`` is the GPU the accumulators live on; None takes the first
    movie's device (the current GPU for a CPU movie).  Nothing touches a device before the first valid ``add``;
    until then ``sum`` and ``sumsq`` are None."""

    def __init__(self, shape, device=None):
        try:
            h, w = (int(s) for s in shape)
        except (TypeError, ValueError):
            raise ValueError(f"shape must be the frame size (h, w), got {shape!r}") from None
        if h < 1 or w < 1:
            raise ValueError(f"shape must be the frame size (h, w), got {shape!r}")
        self.shape = (h, w)
        self.device = None if device is None else torch.device(device)
        self.dtype = None
        self.frames = 0
        self.sum = None
        self.sumsq = None

    @classmethod
    def from_sums(cls, sum, sumsq, frames, dtype):
        """Statistics restored from saved accumulators (int64 (h, w) tensors, kept on the device they are on)."""
        if dtype not in RAW_DTYPES:
            raise ValueError(f"dtype must be torch.uint8 or torch.int16, got {dtype}")
        for name, x in (("sum", sum), ("sumsq", sumsq)):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.int64 or x.dim() != 2:
                raise ValueError(f"{name} must be an int64 (h, w) tensor")
        if sum.shape != sumsq.shape or sum.device != sumsq.device:
            raise ValueError("sum and sumsq must have one shape and one device")
        n = int(frames)
        if not 0 < n <= MAX_FRAMES[dtype]:
            raise ValueError(f"frames must be in 1..{MAX_FRAMES[dtype]}, got {frames!r}")
        st = cls(tuple(sum.shape), sum.device)
        st.dtype, st.frames = dtype, n
        st.sum, st.sumsq = sum.detach().contiguous(), sumsq.detach().contiguous()
        return st

    def _check_more(self, dtype, frames):
        if self.dtype is not None and dtype != self.dtype:
            raise ValueError(f"these statistics hold {self.dtype} frames; {dtype} frames cannot be mixed in")
        if self.frames + frames > MAX_FRAMES[dtype]:
            raise ValueError(f"sumsq (int64) could overflow beyond {MAX_FRAMES[dtype]} {dtype} frames; "
                             f"{self.frames} + {frames} were asked for")

    def add(self, movie):
        """Add the frames of a (t, h, w) or (h, w) uint8 / int16 tensor, from any device.  Returns self."""
        if not isinstance(movie, torch.Tensor) or movie.dtype not in RAW_DTYPES:
            raise ValueError(f"movie must be a uint8 or int16 tensor, got {getattr(movie, 'dtype', type(movie))}")
        if movie.dim() not in (2, 3):
            raise ValueError(f"movie must be (t, h, w) or (h, w), got {tuple(movie.shape)}")
        if tuple(movie.shape[-2:]) != self.shape:
            raise ValueError(f"movie frames are {tuple(movie.shape[-2:])}, these statistics are for {self.shape}")
        t = 1 if movie.dim() == 2 else int(movie.shape[0])
        if t < 1:
            raise ValueError("movie must hold at least one frame")
        self._check_more(movie.dtype, t)
        dev = require_gpu(self.device if self.device is not None else movie.device)
        with device_scope(dev):
            raw = movie.detach().to(dev).contiguous()
            if self.sum is None:
                self.sum = torch.zeros(self.shape, dtype=torch.int64, device=dev)
                self.sumsq = torch.zeros(self.shape, dtype=torch.int64, device=dev)
            elif self.sum.device != dev:
                raise ValueError(f"these statistics live on {self.sum.device}, not on {dev}")
            h, w = self.shape
            check(load().mc_raw_pixel_sums(ptr(raw), int(movie.dtype == torch.int16), t, h, w, ptr(self.sum),
                                           ptr(self.sumsq), stream_ptr(dev)), "mc_raw_pixel_sums")
        self.device, self.dtype = dev, movie.dtype
        self.frames += t
        return self

    def merge(self, other):
        """Add another instance's accumulators (each rank of a sharded session accumulates its own movies; bring
        the tensors together however the session does -- this is a plain tensor add, no collective).  Returns
        self."""
        if not isinstance(other, RawStatistics) or other.shape != self.shape:
            raise ValueError(f"merge takes RawStatistics of frame size {self.shape}")
        if other.frames == 0:
            return self
        self._check_more(other.dtype, other.frames)
        if self.sum is None:
            dev = other.sum.device if self.device is None else self.device
            self.sum, self.sumsq = other.sum.to(dev, copy=True), other.sumsq.to(dev, copy=True)
            self.device = dev
        else:
            self.sum += other.sum.to(self.sum.device)
            self.sumsq += other.sumsq.to(self.sum.device)
        self.dtype = other.dtype
        self.frames += other.frames
        return self


def _check_stats(stats):
    if not isinstance(stats, RawStatistics):
        raise ValueError(f"expected RawStatistics, got {type(stats).__name__}")
    if stats.frames < 1:
        raise ValueError("no frames were added to these statistics")


def estimate_defect_map(stats, hot_factor=5.0, dead_factor=0.2):
    """bool (h, w): the pixels that are wrong in the whole session.  With n = frames and M = (sum of all pixel sums)
    / (n h w) -- the exact integer total, one float64 division -- a pixel p is flagged when

      dead   sum_p <= dead_factor * n * M    (includes sum_p == 0)
      hot    sum_p >= hot_factor * n * M
      stuck  n * sumsq_p == sum_p^2 and n >= 2: zero variance, every frame gave the same value.

    The two thresholds are float64 scalars (the products taken left to right) compared with float64(sum_p), exact
    below 2^53.  The stuck rule is evaluated in integers without forming sum_p^2 (which passes 2^63 after 92 682
    i16 frames): zero variance means sum_p = n v for an integer v and sumsq_p = n v^2, and n v^2 <= sumsq_p fits
    int64 for every frame count RawStatistics accepts."""
    _check_stats(stats)
    hot_factor, dead_factor = float(hot_factor), float(dead_factor)
    if not dead_factor < hot_factor:  # also refuses NaN
        raise ValueError(f"need dead_factor < hot_factor, got {dead_factor!r}, {hot_factor!r}")
    n, (h, w) = stats.frames, stats.shape
    s, q = stats.sum, stats.sumsq
    total = int(s.sum())  # int64: |total| <= 2^15 n h w
    if abs(total) >= EXACT_F64 or int(s.abs().max()) >= EXACT_F64:
        raise ValueError("the pixel sums passed 2^53: the float64 thresholds would no longer be exact")
    mean = float(total) / float(n * h * w)
    sd = s.double()
    defect = (sd <= dead_factor * n * mean) | (sd >= hot_factor * n * mean)
    if n >= 2:
        v = torch.div(s, n, rounding_mode="floor")
        defect |= (v * n == s) & (v * v * n == q)
    return defect


def estimate_gain_reference(stats_or_movies, defect_map=None, return_defect_map=False):
    """fp32 (h, w) gain reference from RawStatistics, or from an iterable of raw movies (accumulated here).

    With good = not defect (``defect_map``: bool (h, w); None calls ``estimate_defect_map``), T = sum of sum_p over
    the good pixels (exact int64) and c = their number:

      gain_p = float32( float64(T) / (float64(c) * float64(sum_p)) )   on good pixels,   0 on defects,

    so gain * (pixel mean) is flat over the good pixels and a defect contributes the frame-independent value 0 to
    every raw route.  T and c * sum_p are required to stay below 2^53, where both conversions and the product are
    exact: the gain is then ONE correctly rounded float64 division, rounded once more to fp32.  ValueError when no
    frames were added, when no pixel is good, or when T or a good pixel's sum is not positive (i16 data around
    zero has no multiplicative gain)."""
    stats = stats_or_movies
    if not isinstance(stats, RawStatistics):
        stats = None
        for movie in [stats_or_movies] if isinstance(stats_or_movies, torch.Tensor) else stats_or_movies:
            if stats is None:
                if not isinstance(movie, torch.Tensor) or movie.dim() not in (2, 3):
                    raise ValueError("movies must be (t, h, w) or (h, w) uint8 / int16 tensors")
                stats = RawStatistics(tuple(movie.shape[-2:]))
            stats.add(movie)
        if stats is None:
            raise ValueError("no frames were added: the iterable of movies is empty")
    _check_stats(stats)
    s = stats.sum
    if defect_map is None:
        defect = estimate_defect_map(stats)
    else:
        if (not isinstance(defect_map, torch.Tensor) or defect_map.dtype != torch.bool
                or tuple(defect_map.shape) != stats.shape):
            raise ValueError(f"defect_map must be a bool {stats.shape} tensor")
        defect = defect_map.to(s.device)
    good = ~defect
    c = int(good.sum())
    if c == 0:
        raise ValueError("no pixel is good: every pixel is in the defect map")
    sg = torch.where(good, s, torch.ones_like(s))  # defects: a harmless divisor
    total, lo, hi = int(torch.where(good, s, torch.zeros_like(s)).sum()), int(sg.min()), int(sg.max())
    if total <= 0 or lo <= 0:
        raise ValueError(f"the good pixels' sums must be positive for a multiplicative gain (total {total}, "
                         f"smallest {lo})")
    if total >= EXACT_F64 or c * hi >= EXACT_F64:
        raise ValueError("T or c * sum_p passed 2^53: the gain would no longer be one exact float64 division")
    num = torch.full(stats.shape, float(total), dtype=torch.float64, device=s.device)
    gain = torch.where(good, (num / (float(c) * sg.double())).float(), torch.zeros((), device=s.device))
    return (gain, defect) if return_defect_map else gain
