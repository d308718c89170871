"""ms per movie and peak device memory of the per-pixel raw statistics (RawStatistics.add: mc_raw_pixel_sums, one
read of the raw bytes) against the obvious torch route at the same commit, in one process, alternated, timed with
device events after warm-up, medians of REPS (3):
  add     RawStatistics.add(movie)          (the accumulators exist; the first add's peak is reported separately)
  torch   movie.sum(0, dtype=torch.int64) and (movie.to(torch.int64) ** 2).sum(0)
Sizes: 4k (40 x 4096^2 u8) and c5 (60 x 8184 x 11520 u8), or SIZES=4k,c5; DTYPE=int16 times i16 movies.  The rate is
the movie's bytes over the time of `add`, to be read against the streaming-copy ceilings of profiles/r03_stream_copy_*.
Both results are compared (torch.equal) before anything is timed.  Prints one JSON line per size."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_motion_correction_amd as mc  # noqa: E402

dev = torch.device("cuda:0")
SIZES = {"4k": (40, 4096, 4096), "c5": (60, 8184, 11520)}
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))
dtype = {"uint8": torch.uint8, "int16": torch.int16}[os.environ.get("DTYPE", "uint8")]


def movie(t, h, w):
    g = torch.Generator(device=dev).manual_seed(5)
    raw = torch.empty((t, h, w), dtype=dtype, device=dev)
    for f in range(t):  # Poisson-like counts, a frame at a time: nothing movie-sized besides the movie
        v = 20.0 + 4.5 * torch.randn((h, w), generator=g, device=dev)
        raw[f] = v.round().clamp(0, 255).to(dtype)
        del v
    return raw


def torch_route(raw):
    return raw.sum(0, dtype=torch.int64), (raw.to(torch.int64) ** 2).sum(0)


for name in os.environ.get("SIZES", "4k,c5").split(","):
    t, h, w = SIZES[name]
    raw = movie(t, h, w)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    stats = mc.RawStatistics((h, w)).add(raw)  # the first add allocates the two accumulators, 16 B per pixel
    torch.cuda.synchronize()
    first_peak = (torch.cuda.max_memory_allocated() - base) / 1e9
    s, q = torch_route(raw)
    assert torch.equal(stats.sum, s) and torch.equal(stats.sumsq, q)
    del s, q
    routes = {"add": lambda: stats.add(raw), "torch": lambda: torch_route(raw)}
    for _ in range(warm):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    peak = {}
    for _ in range(reps):
        for key, fn in routes.items():
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            b.synchronize()
            ms[key].append(a.elapsed_time(b))
            peak[key] = (torch.cuda.max_memory_allocated() - base) / 1e9
            del out
    nbytes = raw.numel() * raw.element_size()
    res = {"size": f"{t}x{h}x{w}", "dtype": str(dtype), "movie_gb": round(nbytes / 1e9, 3)}
    for k, v in ms.items():
        res[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
                  "peak_gb_above_inputs": round(peak[k], 3)}
    res["add_tb_per_s"] = round(nbytes / (statistics.median(ms["add"]) * 1e-3) / 1e12, 3)
    res["first_add_peak_gb_above_inputs"] = round(first_peak, 3)
    res["frames_accumulated"] = stats.frames
    res["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(res), flush=True)
    del raw, stats, routes
    torch.cuda.empty_cache()
