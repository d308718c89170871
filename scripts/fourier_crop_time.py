"""ms per movie and peak device memory of Fourier cropping (2x binning) a raw u8 movie with a gain reference, and of the
session's first step with and without it, in one process, alternated, timed with device events after warm-up:
  crop_fused   fourier_crop_raw(raw, gain)                          (no full-size fp32 movie)
  crop_comp    fourier_crop(condition_movie(raw, gain))
  binned       motion_correct_raw_binned(raw, gain, ps, dose_per_frame=1.0, return_plain_sum=True)
               (crop, then the estimate and both sums at half size)
  full         motion_correct_raw_fast(raw, gain, ps, dose_per_frame=1.0, return_plain_sum=True)
               (today's route: everything at full size)
Sizes: 4k (40 x 4096^2) and C5 (60 x 8184 x 11520), or SIZES=4k,c5; ROUTES=crop_fused,crop_comp,binned,full picks the
routes (a kernel trace of one route).  Prints one JSON line per size."""
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
DOSE, PS = 1.0, 0.5


def movie(t, h, w):
    g = torch.Generator(device=dev).manual_seed(5)
    base = torch.rand((h + 32, w + 32), generator=g, device=dev) * 40 + 10
    raw = torch.empty((t, h, w), dtype=torch.uint8, device=dev)
    for f in range(t):
        dy, dx = 2 * ((f * 3) // t), 2 * ((f * 5) // t)
        noise = torch.randn((h, w), generator=g, device=dev) * 4
        raw[f] = (base[16 + dy:16 + dy + h, 16 - dx:16 - dx + w] + noise).round().clamp(0, 255).to(torch.uint8)
        del noise
    gain = (1.0 + 0.1 * torch.randn((h, w), generator=g, device=dev)).clamp(0.5, 1.5)
    return raw, gain


want = os.environ.get("ROUTES", "crop_fused,crop_comp,binned,full").split(",")
for name in os.environ.get("SIZES", "4k,c5").split(","):
    t, h, w = SIZES[name]
    raw, gain = movie(t, h, w)
    routes = {"crop_fused": lambda: mc.fourier_crop_raw(raw, gain),
              "crop_comp": lambda: mc.fourier_crop(mc.condition_movie(raw, gain)),
              "binned": lambda: mc.motion_correct_raw_binned(raw, gain, PS, dose_per_frame=DOSE, return_plain_sum=True),
              "full": lambda: mc.motion_correct_raw_fast(raw, gain, PS, dose_per_frame=DOSE, return_plain_sum=True)}
    routes = {k: v for k, v in routes.items() if k in want}
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
    res = {"size": f"{t}x{h}x{w}", "input_gb": round((raw.numel() + gain.numel() * 4) / 1e9, 2)}
    for k, v in ms.items():
        res[k] = {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2),
                  "peak_gb_above_inputs": round(peak[k], 2)}
    res["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(res), flush=True)
    del raw, gain, routes
    torch.cuda.empty_cache()
