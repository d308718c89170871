"""ms per movie and peak device memory of two routes to the example's whole-image images -- the dose-weighted sum
and the plain sum of the Fourier-shifted frames -- of a raw u8 movie with a gain reference and a rigid field, in one
process, alternated, timed with device events after warm-up:
  fused   motion_correct_sum_fast_raw(raw, gain, field, 1.0, dose_per_frame=1.0, return_plain_sum=True)
          (no conditioned and no shifted fp32 movie)
  comp    condition_movie(raw, gain) -> correct_motion_fast(img, field) -> .sum(0) and dose_weighted_sum
Sizes: 4k (40 x 4096^2), C3 (40 x 4092 x 5760) and C5 (60 x 8184 x 11520), or SIZES=4k,c3,c5; ROUTES=fused,comp
picks the routes (a kernel trace of one route).  Prints one JSON line per size."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_motion_correction_amd as mc  # noqa: E402

dev = torch.device("cuda:0")
SIZES = {"4k": (40, 4096, 4096), "c3": (40, 4092, 5760), "c5": (60, 8184, 11520)}
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))
DOSE = 1.0


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


def field_for(t):
    """a rigid drift of a few pixels with sub-pixel parts, (2, t, 1, 1)"""
    tt = torch.linspace(-1, 1, t)
    return torch.stack([2.7 * tt, -3.2 * tt])[:, :, None, None].contiguous().to(dev)


def comp(raw, gain, field):
    img = mc.condition_movie(raw, gain)
    cor = mc.correct_motion_fast(img, field.clone())
    del img
    return mc.dose_weighted_sum(cor, 1.0, DOSE), cor.sum(0)


want = os.environ.get("ROUTES", "fused,comp").split(",")
for name in os.environ.get("SIZES", "4k,c3,c5").split(","):
    t, h, w = SIZES[name]
    raw, gain = movie(t, h, w)
    field = field_for(t)
    routes = {"fused": lambda: mc.motion_correct_sum_fast_raw(raw, gain, field, 1.0, dose_per_frame=DOSE,
                                                              return_plain_sum=True),
              "comp": lambda: comp(raw, gain, field)}
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
