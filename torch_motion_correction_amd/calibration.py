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

The defect map is then used to REPAIR the movies (MotionCor2 -DefectFile / -DefectMap, RELION --defect_file), as a
raw movie -> raw movie stage in front of any raw route and a matching gain -> gain step:

  DefectFill                  the plan of a defect map: the defect list and each defect's donor pixels
  fill_defects_raw            every defect of every frame replaced by one of its donors, chosen by a hash of (seed,
                              frame, defect): an exact element of the movie's own type with the movie's own noise
  fill_defects_gain           the defects' gains replaced by the mean gain of their donors
  defect_map_from_rectangles  MotionCor2 defect-file entries (x, y, width, height) -> a bool map, on the host

csrc/defect_fill.hip holds the kernels, tests/defect_reference.py restates the rule with Python integers.
"""

from __future__ import annotations

import operator

import torch

from . import _lib
from ._lib import check, device_scope, load, ptr, require_gpu, stream_ptr

RAW_DTYPES = (torch.uint8, torch.int16)
# sumsq is exposed as int64: after n frames it is at most 255^2 n (u8) or 2^30 n (i16, all -32768), which passes
# 2^63 - 1 beyond these frame counts.  add() and merge() refuse the frames that would exceed them.
MAX_FRAMES = {torch.uint8: (2**63 - 1) // 255**2, torch.int16: (2**63 - 1) // 2**30}
EXACT_F64 = 2**53  # integers below it convert to float64 exactly
FILL_DTYPES = (torch.uint8, torch.int16, torch.float16, torch.float32)  # 1, 2, 2 and 4 bytes: the fill copies bits
MAX_REACH = 16


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


# ------------------------------------------------------------------ defects filled from the map


def _check_defect_map(defect_map, what="defect_map"):
    if (not isinstance(defect_map, torch.Tensor) or defect_map.dtype != torch.bool or defect_map.dim() != 2
            or defect_map.numel() < 1):
        raise ValueError(f"{what} must be a bool (h, w) tensor, got "
                         f"{getattr(defect_map, 'dtype', type(defect_map).__name__)} "
                         f"{tuple(getattr(defect_map, 'shape', ()))}")
    if defect_map.numel() >= 2**31:
        raise ValueError(f"{what}: frames of 2^31 pixels and more are not supported")


def _check_reach(reach):
    if isinstance(reach, bool) or not isinstance(reach, int) or not 1 <= reach <= MAX_REACH:
        raise ValueError(f"reach must be an int in 1..{MAX_REACH}, got {reach!r}")
    return reach


class DefectFill:
    """The fill plan of a bool (h, w) ``defect_map``.  With the defects listed in row-major order (``j`` a defect's
    place in the list) and the ring at Chebyshev distance r around a defect = the pixels with max(|dy|, |dx|) == r
    inside the frame, defect j's donors are the good pixels of the FIRST ring r = 1 .. ``reach`` that holds any, in
    row-major order (at most 8 r of them).

      pixels (n,)             the defects' linear indices y * w + x, int32, ascending
      donors (n, 8 * reach)   the donors' linear indices, int32, unused entries -1
      counts (n,)             the number of donors, int32
      shape, reach, n, device

    The tables live on ``device`` (None: the map's device, the current GPU for a CPU map); mc_defect_donors
    (csrc/defect_fill.hip) writes them, one thread per defect.  A defect without a good pixel within ``reach`` is a
    ValueError naming the first such pixel as (y, x) and the reach -- from one device-to-host read of
    ``counts.min()``, here, before any movie is touched.  A map without defects is valid and fills nothing."""

    def __init__(self, defect_map, reach=4, device=None):
        _check_defect_map(defect_map)
        self.reach = _check_reach(reach)
        h, w = (int(s) for s in defect_map.shape)
        self.shape = (h, w)
        dev = require_gpu(device if device is not None else defect_map.device)
        with device_scope(dev):
            dmap = defect_map.detach().to(dev).contiguous()
            # torch.nonzero lists the indices in row-major order
            self.pixels = torch.nonzero(dmap.reshape(-1)).reshape(-1).to(torch.int32)
            n = int(self.pixels.numel())
            self.donors = torch.empty((n, 8 * self.reach), dtype=torch.int32, device=dev)
            self.counts = torch.empty((n,), dtype=torch.int32, device=dev)
            if n:
                check(_lib.load().mc_defect_donors(ptr(dmap.view(torch.uint8)), h, w, ptr(self.pixels), n,
                                                   self.reach, ptr(self.donors), ptr(self.counts), stream_ptr(dev)),
                      "mc_defect_donors")
                if int(self.counts.min()) == 0:
                    p = int(self.pixels[int(torch.nonzero(self.counts == 0)[0])])
                    raise ValueError(f"defect pixel (y, x) = ({p // w}, {p % w}) has no good pixel within "
                                     f"reach={self.reach}: raise reach or mask the region another way")
        self.n, self.device = n, dev


def _check_fill(fill, frame_shape, what):
    """The argument rules of `fill` (a DefectFill or a bool map) against an (h, w) of a movie or a gain."""
    if isinstance(fill, DefectFill):
        shape = fill.shape
    else:
        _check_defect_map(fill, "fill (a DefectFill or a defect map)")
        shape = tuple(int(s) for s in fill.shape)
    if shape != tuple(int(s) for s in frame_shape):
        raise ValueError(f"the defect map has shape {shape}, the {what} {tuple(frame_shape)}")


def _fill_plan(fill, data, device):
    """-> the DefectFill of `fill` for `data` (a movie or a gain).  A plan decides the device; a map's plan is built
    on `device`, else on the data's device."""
    if isinstance(fill, DefectFill):
        if device is not None and require_gpu(device) != fill.device:
            raise ValueError(f"the DefectFill lives on {fill.device}, {torch.device(device)} was asked for")
        return fill
    return DefectFill(fill, device=device if device is not None else data.device)


def fill_defects_raw(movie, fill, seed=0, in_place=False, device=None):
    """A (t, h, w) or (h, w) movie of uint8, int16, float16 or float32 with its detector defects filled: for frame f
    and defect j (``DefectFill``'s list)

      x = seed ^ (f * 0x9E3779B1) ^ (j * 0x85EBCA77)                                  uint32, wrapping
      x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16
      out[f, p_j] = movie[f, donors[j, (x * count_j) >> 32]]

    -- a deterministic "random" pick among the nearest good pixels, as MotionCor2 and RELION fill defects.  The value
    is an exact element of the movie (its bits are copied) with the movie's own noise; a neighbour mean would
    imprint a low-variance pattern.  Every other element equals ``movie`` bit for bit.  The result has the movie's
    dtype and shape and is a raw movie for every ``*_raw*`` function, ``condition_movie``, the pipelines and
    ``RawStatistics``; use it with ``fill_defects_gain`` of the same plan.

    ``fill``: a ``DefectFill``, or a bool (h, w) map from which one is built with the default reach.  ``seed``: an
    int in 0 .. 2^32 - 1.  ``in_place=True`` needs a contiguous movie that is already on the GPU and returns that
    tensor; otherwise the movie is copied (the one full pass: the defect list is sparse) and the copy is filled
    (mc_raw_fill_defects, one thread per frame and defect), and the result comes back on the movie's device.
    Argument errors are ValueErrors raised before any device is touched."""
    if not isinstance(movie, torch.Tensor) or movie.dtype not in FILL_DTYPES:
        raise ValueError("movie must be a uint8, int16, float16 or float32 tensor, got "
                         f"{getattr(movie, 'dtype', type(movie).__name__)}")
    if movie.dim() not in (2, 3) or movie.numel() < 1:
        raise ValueError(f"movie must be (t, h, w) or (h, w) with at least one frame, got {tuple(movie.shape)}")
    _check_fill(fill, movie.shape[-2:], "movie's frames")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2**32:
        raise ValueError(f"seed must be an int in 0..2^32-1, got {seed!r}")
    if in_place and not (movie.is_cuda and movie.is_contiguous()):
        raise ValueError("in_place=True needs a contiguous movie that is already on the GPU")
    plan = _fill_plan(fill, movie, movie.device if in_place else device)  # in place: the movie's device
    dev = plan.device
    t = 1 if movie.dim() == 2 else int(movie.shape[0])
    h, w = plan.shape
    with device_scope(dev):
        if in_place:
            out = movie
        else:
            out = torch.empty(movie.shape, dtype=movie.dtype, device=dev)
            out.copy_(movie.detach())
        if plan.n:
            check(_lib.load().mc_raw_fill_defects(ptr(out), out.element_size(), t, h, w, ptr(plan.pixels),
                                                  ptr(plan.donors), ptr(plan.counts), plan.n, plan.reach, seed,
                                                  stream_ptr(dev)), "mc_raw_fill_defects")
        return out if in_place else out.to(movie.device)


def fill_defects_gain(gain, fill, device=None):
    """The fp32 (h, w) gain reference for a movie filled by ``fill_defects_raw``: a new tensor with

      gain'[p_j] = float32( sum_k float64(gain[donors[j, k]]) / count_j )     (the sum in table order)

    at the defects and ``gain`` bit for bit elsewhere.  A filled pixel carries a donor's raw value, so it needs a
    gain of the donors' size: with ``estimate_gain_reference``'s gain (0 at defects, positive on good pixels) every
    filled pixel gets a positive one.  ``fill`` as in ``fill_defects_raw``; argument errors are ValueErrors raised
    before any device is touched; the result comes back on the gain's device."""
    if not isinstance(gain, torch.Tensor) or gain.dtype != torch.float32 or gain.dim() != 2 or gain.numel() < 1:
        raise ValueError("gain must be a float32 (h, w) tensor, got "
                         f"{getattr(gain, 'dtype', type(gain).__name__)} {tuple(getattr(gain, 'shape', ()))}")
    _check_fill(fill, gain.shape, "gain")
    plan = _fill_plan(fill, gain, device)
    dev = plan.device
    h, w = plan.shape
    with device_scope(dev):
        out = torch.empty((h, w), dtype=torch.float32, device=dev)
        out.copy_(gain.detach())
        if plan.n:
            check(_lib.load().mc_gain_fill_defects(ptr(out), h, w, ptr(plan.pixels), ptr(plan.donors),
                                                   ptr(plan.counts), plan.n, plan.reach, stream_ptr(dev)),
                  "mc_gain_fill_defects")
        return out.to(gain.device)


def defect_map_from_rectangles(shape, rectangles):
    """bool (h, w) CPU map from MotionCor2 defect-file entries: ``rectangles`` is an iterable of (x, y, width,
    height) in pixels, x along the rows' direction (columns x .. x + width - 1, rows y .. y + height - 1 are
    defects).  ``shape`` is the frame size (h, w).  ValueError for an entry that is not four integers, for an empty
    rectangle (width or height < 1) and for one that leaves the frame.  Host only."""
    try:
        h, w = (operator.index(s) for s in shape)
    except (TypeError, ValueError):
        raise ValueError(f"shape must be the frame size (h, w), got {shape!r}") from None
    if h < 1 or w < 1:
        raise ValueError(f"shape must be the frame size (h, w), got {shape!r}")
    out = torch.zeros((h, w), dtype=torch.bool)
    for i, rect in enumerate(rectangles):
        try:
            if any(isinstance(v, bool) for v in rect):
                raise TypeError
            x, y, rw, rh = (operator.index(v) for v in rect)
        except (TypeError, ValueError):
            raise ValueError(f"rectangle {i} must be four integers (x, y, width, height), got {rect!r}") from None
        if rw < 1 or rh < 1:
            raise ValueError(f"rectangle {i} is empty: (x, y, width, height) = {(x, y, rw, rh)}")
        if x < 0 or y < 0 or x + rw > w or y + rh > h:
            raise ValueError(f"rectangle {i} leaves the {(h, w)} frame: (x, y, width, height) = {(x, y, rw, rh)}")
        out[y:y + rh, x:x + rw] = True
    return out
