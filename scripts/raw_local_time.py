"""ms per movie and peak device memory of two routes for the local-motion flow of a raw u8 movie with a gain
reference, in one process, alternated, timed with device events after warm-up:
  fused   motion_correct_raw_patches(raw, gain, 1.0)                                   (no fp32 movie)
  cond    condition_movie(raw, gain) + estimate_motion_cross_correlation_patches + motion_correct_sum
Sizes: C3 (40 x 4092 x 5760) and C5 (60 x 8184 x 11520), or SIZES=c3 / c5.  The movie is a drifting texture
(shifted copies of one random image), so the estimator finds real peaks.  Prints one JSON line per size."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_motion_correction_amd as mc  # noqa: E402

dev = torch.device("cuda:0")
SIZES = {"c3": (40, 4092, 5760), "c5": (60, 8184, 11520)}
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))


def movie(t, h, w):
    g = torch.Generator(device=dev).manual_seed(5)
    base = torch.rand((h + 32, w + 32), generator=g, device=dev) * 40 + 10
    raw = torch.empty((t, h, w), dtype=torch.uint8, device=dev)
    for f in range(t):
        dy, dx = (f * 3) // t, (f * 5) // t
        noise = torch.randn((h, w), generator=g, device=dev) * 4
        raw[f] = (base[16 + dy:16 + dy + h, 16 - dx:16 - dx + w] + noise).round().clamp(0, 255).to(torch.uint8)
        del noise
    gain = (1.0 + 0.1 * torch.randn((h, w), generator=g, device=dev)).clamp(0.5, 1.5)
    return raw, gain


def cond(raw, gain):
    img = mc.condition_movie(raw, gain)
    field, pos = mc.estimate_motion_cross_correlation_patches(img, 1.0, patch_sidelength=1024)
    return field, pos, mc.motion_correct_sum(img, field, 1.0)


for name in os.environ.get("SIZES", "c3,c5").split(","):
    t, h, w = SIZES[name]
    raw, gain = movie(t, h, w)
    routes = {"fused": lambda: mc.motion_correct_raw_patches(raw, gain, 1.0), "cond": lambda: cond(raw, gain)}
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
