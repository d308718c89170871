"""Movie-level software pipeline on one GPU.

The reference processes one movie at a time: estimate_global_motion -> correct_motion
(-> sum) (examples/ttMotion.py:284-398).  Movies are independent, so when several are
processed back to back the estimator of movie k+1 (latency- and issue-bound FFT kernels)
can run on a second HIP stream underneath the HBM-bound warp of movie k.  Results are
identical to calling the two API functions one after the other; only the enqueue order
differs.  No host synchronisation happens here: the caller's stream waits on both
pipeline streams at the end of ``run``.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Iterable, Optional

import torch

from . import engine
from ._lib import device_scope, require_gpu


@dataclass
class MovieResult:
    field: torch.Tensor  # (2, t, 1, 1) Angstrom, as estimate_global_motion returns it
    total: torch.Tensor  # (h, w) sum of the corrected frames
    frames: Optional[torch.Tensor]  # (t, h, w) corrected frames or None


class MoviePipeline:
    """estimate_global_motion -> correct_motion (+ fused frame sum) over a sequence of
    movies, two HIP streams deep.  Arguments mirror estimate_global_motion
    (estimate_motion_xc.py:21-28) and correct_motion (correct_motion.py:18-25)."""

    def __init__(self, device=None, pixel_spacing: float = 1.0, reference_frame: Optional[int] = None,
                 b_factor: float = 500, frequency_range=(300, 10), grid_type: str = "catmull_rom",
                 return_frames: bool = True, overlap: bool = True):
        self.device = require_gpu(device)
        self.pixel_spacing = float(pixel_spacing)
        self.reference_frame = reference_frame
        self.b_factor = float(b_factor)
        self.frequency_range = tuple(frequency_range)
        self.grid_type = grid_type
        self.return_frames = return_frames
        self.overlap = overlap
        # the estimator's stream gets the higher priority: its short, latency-bound kernels then
        # slot in between the waves of the long HBM-bound warp instead of queueing behind them
        # (measured: 19.4-19.7 k -> 20.1-20.4 k frames/s on 40 x 4096^2 stacks)
        self._s_est = torch.cuda.Stream(self.device, priority=-1) if overlap else None
        self._s_warp = torch.cuda.Stream(self.device, priority=0) if overlap else None

    # the two stages, each enqueued on whatever stream is current
    def _estimate(self, img: torch.Tensor, after_k1: Optional[Callable[[], None]] = None):
        """-> ((2,t,1,1) Angstrom field (dfu.py:129-162), warp_args for ``_correct``).  Everything of
        correct_motion that only needs the field -- the per-frame lattice values and the rigid warp's weight
        tables -- is built right here, on the ESTIMATOR's stream, in two launches (mc_rigid_tables_from_shifts;
        it used to be seven, each waiting for a wave slot under the previous movie's warp).  Every tensor in
        warp_args is record_stream()ed on the warp stream.  `after_k1()` runs once K1 is enqueued."""
        t = img.shape[0]
        ref = t // 2 if self.reference_frame is None else int(self.reference_frame)
        shifts = engine.global_shifts(img, ref, self.pixel_spacing, self.b_factor, self.frequency_range, after_k1)
        return engine.rigid_tables_from_shifts(shifts, tuple(img.shape), self.pixel_spacing, self.grid_type)

    def _correct(self, img: torch.Tensor, warp_args):
        return engine.warp(img, None, self.pixel_spacing, want_frames=self.return_frames, want_sum=True,
                           rigid=True, tables=warp_args)

    def iterate(self, movies: Iterable[torch.Tensor],
                around_warp: Optional[Callable[[Callable[[], object]], object]] = None):
        """Generator form of ``run``: yields a MovieResult as soon as the movie's work has been
        ENQUEUED.  A yielded result is ordered on the pipeline's warp stream; the caller's
        stream only waits for the pipeline once the generator is exhausted, so use the tensors
        after the loop (or drop them: memory returns to the warp stream's pool, which the
        next movie reuses).  `around_warp(fn)` (optional, for instrumentation) must call fn()
        and return its result; it runs with the warp stream current."""
        dev = self.device
        call = around_warp if around_warp is not None else (lambda fn: fn())
        # every enqueue happens with the pipeline's GPU as the current HIP device (libmcorr launches
        # on the current device); the scope is left again before control returns to the caller
        if not self.overlap:
            for img in movies:
                with device_scope(dev):
                    img = self._check(img)
                    field, warp_args = self._estimate(img)
                    frames, total = call(lambda: self._correct(img, warp_args))
                yield MovieResult(field, total, frames)
            return
        with device_scope(dev):
            caller = torch.cuda.current_stream(dev)
            start = torch.cuda.Event()
            start.record(caller)
            self._s_est.wait_event(start)
            self._s_warp.wait_event(start)

        def enqueue_warp(img, field, warp_args, ready, next_k1_done):
            # the warp of movie k waits for its estimate and, when there is one, for movie k+1's K1
            # (which has then left the HBM to this warp)
            with torch.cuda.stream(self._s_warp):
                self._s_warp.wait_event(ready)
                if next_k1_done is not None:
                    self._s_warp.wait_event(next_k1_done)
                field.record_stream(self._s_warp)
                for x in warp_args:
                    if isinstance(x, torch.Tensor):
                        x.record_stream(self._s_warp)
                frames, total = call(lambda: self._correct(img, warp_args))
            return MovieResult(field, total, frames)

        try:
            pending = None  # (img, field, warp_args, ready) of the movie whose warp is not enqueued yet
            for img in movies:
                res = None
                with device_scope(dev):
                    img = self._check(img)
                    img.record_stream(self._s_est)
                    img.record_stream(self._s_warp)
                    k1_done = torch.cuda.Event()
                    with torch.cuda.stream(self._s_est):
                        field, warp_args = self._estimate(img, lambda: k1_done.record(self._s_est))
                        ready = torch.cuda.Event()
                        ready.record(self._s_est)
                    if pending is not None:
                        res = enqueue_warp(*pending, k1_done)
                    pending = (img, field, warp_args, ready)
                if res is not None:
                    yield res
            if pending is not None:
                with device_scope(dev):
                    res = enqueue_warp(*pending, None)
                yield res
        finally:
            with device_scope(dev):
                for s in (self._s_est, self._s_warp):
                    done = torch.cuda.Event()
                    done.record(s)
                    caller.wait_event(done)

    def run(self, movies: Iterable[torch.Tensor],
            around_warp: Optional[Callable[[Callable[[], object]], object]] = None) -> list[MovieResult]:
        """Process `movies` ((t,h,w) float32 or float16 tensors on the pipeline's device) in order and
        return every result, ready for use on the caller's current stream."""
        results = list(self.iterate(movies, around_warp))
        if self.overlap:
            caller = torch.cuda.current_stream(self.device)
            for r in results:
                for x in (r.field, r.total, r.frames):
                    if x is not None:
                        x.record_stream(caller)
        return results

    def _check(self, img: torch.Tensor) -> torch.Tensor:
        if img.dim() != 3:
            raise ValueError(f"expected a (t, h, w) stack, got shape {tuple(img.shape)}")
        # fp16 stacks stay fp16: K1 (4096-column frames) and the rigid warp read the 16-bit samples
        dtype = torch.float16 if img.dtype == torch.float16 else torch.float32
        if img.device != self.device or img.dtype != dtype or not img.is_contiguous():
            img = img.detach().to(device=self.device, dtype=dtype).contiguous()
        return img


class RawMoviePipeline(MoviePipeline):
    """The same two-stream pipeline for RAW uint8 / int16 movies and a gain reference (N2): per movie one
    statistics pass over the raw bytes, then the estimator's row transform and the rigid warp condition the
    samples on the fly (``raw * gain - frame mean``, examples/ttMotion.py:90-121, 180-199) -- no conditioned
    fp32 movie is allocated.  Results equal ``condition_movie`` followed by the MoviePipeline.  Frame shapes
    without a fused kernel raise McorrUnsupported (use ``motion_correct_raw``, which falls back).

    ``hot_pixel_threshold``: the example's hot-pixel step as in ``motion_correct_raw`` (per movie the same
    results).  The length of a movie's hot-pixel list is read back to the host once, right after its detection
    pass on the estimator's stream and before its K1 is enqueued (the previous movie's warp is then not yet
    enqueued; the one before it may still run).  A movie with more hot pixels than the list holds raises
    McorrUnsupported naming the threshold."""

    def __init__(self, gain, device=None, pixel_spacing: float = 1.0, reference_frame: Optional[int] = None,
                 b_factor: float = 500, frequency_range=(300, 10), grid_type: str = "catmull_rom",
                 return_frames: bool = True, overlap: bool = True, mean_zero: bool = True,
                 hot_pixel_threshold: Optional[float] = None):
        self.hot_pixel_threshold = engine.check_hot_pixel_threshold(hot_pixel_threshold)
        super().__init__(device, pixel_spacing, reference_frame, b_factor, frequency_range, grid_type,
                         return_frames, overlap)
        self.gain = None if gain is None else gain.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self.mean_zero = bool(mean_zero)

    def _check(self, img: torch.Tensor) -> torch.Tensor:
        if img.dim() != 3:
            raise ValueError(f"expected a (t, h, w) stack, got shape {tuple(img.shape)}")
        if img.dtype not in (torch.uint8, torch.int16):
            raise TypeError(f"RawMoviePipeline reads uint8 or int16 movies, got {img.dtype}")
        if img.device != self.device or not img.is_contiguous():
            img = img.detach().to(device=self.device).contiguous()
        return img

    def _estimate(self, img: torch.Tensor, after_k1: Optional[Callable[[], None]] = None):
        t = img.shape[0]
        ref = t // 2 if self.reference_frame is None else int(self.reference_frame)
        # the statistics (and hot-pixel) passes, on the estimator's stream
        rm = engine.RawMovie(img, self.gain, mean_zero=self.mean_zero, hot_pixel_threshold=self.hot_pixel_threshold)
        shifts = engine.global_shifts_raw(rm, ref, self.pixel_spacing, self.b_factor, self.frequency_range, after_k1)
        field, (shifts_px, scratch) = engine.rigid_tables_from_shifts(shifts, tuple(img.shape), self.pixel_spacing,
                                                                      self.grid_type)
        # every tensor the warp stream reads that was made on the estimator's stream (the all-ones gain of
        # gain=None, the hot-pixel list, ...) is in the tuple: iterate() record_stream()s them all
        return field, (shifts_px, scratch, *rm.device_tensors(), rm)

    def _correct(self, img: torch.Tensor, warp_args):
        shifts_px, scratch, rm = warp_args[0], warp_args[1], warp_args[-1]
        return engine.warp_rigid_raw(rm, None, self.pixel_spacing, want_frames=self.return_frames, want_sum=True,
                                     tables=(shifts_px, scratch))


def motion_correct_movies(movies: Iterable[torch.Tensor], pixel_spacing: float, reference_frame=None,
                          b_factor=500, frequency_range=(300, 10), grid_type="catmull_rom",
                          return_frames=False, device=None, overlap=True) -> list[MovieResult]:
    """Global (rigid) motion correction of several movies: for each one the field of
    estimate_global_motion and the aligned frame sum (and the corrected frames when asked).
    Equivalent to ``[ (f := estimate_global_motion(m, ps, ...), motion_correct_sum(m, f, ps)) ]``
    with the two stages of consecutive movies overlapped on the GPU."""
    first = None
    movies = list(movies)
    if movies:
        first = movies[0]
    dev = require_gpu(device if device is not None else (first.device if first is not None else None))
    pipe = MoviePipeline(dev, pixel_spacing, reference_frame, b_factor, frequency_range, grid_type,
                         return_frames, overlap)
    return pipe.run(movies)
