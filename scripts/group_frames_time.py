"""ms per movie and peak device memory of the rolling frame-group sums (group_frames_raw: mc_raw_group_frames, one
streaming pass) against the torch composition at the same commit, in one process, alternated, timed with device
events after warm-up, medians of REPS (3):
  group   group_frames_raw(movie, g)
  torch   the windowed sum of movie.to(torch.int32), narrowed to int16
Sizes: 4k (40 x 4096^2 u8) and c5 (60 x 8184 x 11520 u8), or SIZES=4k,c5; GROUPS=3,8; DTYPE=int16 times i16 movies.
The rate is the compulsory bytes -- one read of the movie and one write of the int16 output -- over the time of
`group`, to be read against the streaming-copy ceilings of profiles/r03_stream_copy_*.  Both results are compared
(torch.equal) before anything is timed.  Prints one JSON line per size and group."""
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
groups = [int(g) for g in os.environ.get("GROUPS", "3,8").split(",")]


def movie(t, h, w):
    g = torch.Generator(device=dev).manual_seed(5)
    raw = torch.empty((t, h, w), dtype=dtype, device=dev)
    for f in range(t):  # Poisson-like counts, a frame at a time: nothing movie-sized besides the movie
        v = 20.0 + 4.5 * torch.randn((h, w), generator=g, device=dev)
        raw[f] = v.round().clamp(0, 255).to(dtype)
        del v
    return raw


def torch_route(raw, group):
    t = raw.shape[0]
    wide = raw.to(torch.int32)
    out = torch.zeros_like(wide)
    for d in range(-((group - 1) // 2), group // 2 + 1):  # out[i] += wide[i + d] where that frame exists
        a, b = max(0, -d), min(t, t - d)
        if a < b:
            out[a:b] += wide[a + d:b + d]
    return out.to(torch.int16)


for name in os.environ.get("SIZES", "4k,c5").split(","):
    t, h, w = SIZES[name]
    raw = movie(t, h, w)
    for group in groups:
        got, want = mc.group_frames_raw(raw, group), torch_route(raw, group)
        assert torch.equal(got, want)
        del got, want
        routes = {"group": lambda: mc.group_frames_raw(raw, group), "torch": lambda: torch_route(raw, group)}
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
        nbytes = raw.numel() * (raw.element_size() + 2)
        res = {"size": f"{t}x{h}x{w}", "dtype": str(dtype), "group_frames": group, "compulsory_gb": round(nbytes / 1e9, 3)}
        for k, v in ms.items():
            res[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
                      "peak_gb_above_inputs": round(peak[k], 3)}
        res["group_tb_per_s"] = round(nbytes / (statistics.median(ms["group"]) * 1e-3) / 1e12, 3)
        res["device"] = torch.cuda.get_device_name(dev)
        print(json.dumps(res), flush=True)
        del routes
        torch.cuda.empty_cache()
    del raw
    torch.cuda.empty_cache()
