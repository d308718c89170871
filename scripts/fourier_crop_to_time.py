"""ms per movie and peak device memory of Fourier cropping to a given size, in one process, alternated, timed with device
events after warm-up, medians of REPS (3):
  crop_to      fourier_crop_to(fp32 movie, shape)
  torch_fft    the same definition written with torch.fft.rfft2 / irfft2 on the device, a frame at a time
  raw_fused    fourier_crop_to_raw(u8 movie, gain, shape)                  (no full-size fp32 movie)
  raw_comp     fourier_crop_to(condition_movie(u8 movie, gain), shape)
Sizes: k3 (40 x 4092 x 5760 -> 2046 x 2880, a K3 counting-mode movie by 2) and c5 (60 x 8184 x 11520 -> 5456 x 7680, a
super-resolution movie by 1.5), or SIZES=k3,c5; ROUTES=crop_to,torch_fft,raw_fused,raw_comp picks the routes.  Peak
memory is what a route allocates above its inputs.  Prints one JSON line per size."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_motion_correction_amd as mc  # noqa: E402

dev = torch.device("cuda:0")
SIZES = {"k3": ((40, 4092, 5760), (2046, 2880)), "c5": ((60, 8184, 11520), (5456, 7680))}
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))


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


def torch_crop_to(x, shape):
    """The definition with torch's transforms, frame by frame (one full-size spectrum at a time)."""
    h2, w2 = shape
    h = x.shape[1]
    out = torch.empty((x.shape[0], h2, w2), dtype=torch.float32, device=x.device)
    for f in range(x.shape[0]):
        F = torch.fft.rfft2(x[f])
        out[f] = torch.fft.irfft2(torch.cat((F[: h2 // 2, : w2 // 2 + 1], F[h - h2 // 2:, : w2 // 2 + 1])), s=(h2, w2))
    return out


want = os.environ.get("ROUTES", "crop_to,torch_fft,raw_fused,raw_comp").split(",")
for name in os.environ.get("SIZES", "k3,c5").split(","):
    (t, h, w), shape = SIZES[name]
    raw, gain = movie(t, h, w)
    x = mc.condition_movie(raw, gain) if {"crop_to", "torch_fft"} & set(want) else None
    routes = {"crop_to": lambda: mc.fourier_crop_to(x, shape),
              "torch_fft": lambda: torch_crop_to(x, shape),
              "raw_fused": lambda: mc.fourier_crop_to_raw(raw, gain, shape),
              "raw_comp": lambda: mc.fourier_crop_to(mc.condition_movie(raw, gain), shape)}
    routes = {k: v for k, v in routes.items() if k in want}
    res = {"size": f"{t}x{h}x{w}", "to": f"{shape[0]}x{shape[1]}",
           "input_gb": {"u8_and_gain": round((raw.numel() + gain.numel() * 4) / 1e9, 2),
                        "fp32": None if x is None else round(x.numel() * 4 / 1e9, 2)}}
    if "crop_to" in routes and "torch_fft" in routes:  # what is timed is the same thing
        a, b = routes["crop_to"](), routes["torch_fft"]()
        res["max_abs_diff_over_range"] = float((a - b).abs().max() / (b.max() - b.min()))
        del a, b
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
    for k, v in ms.items():
        res[k] = {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2),
                  "peak_gb_above_inputs": round(peak[k], 2)}
    res["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(res), flush=True)
    del raw, gain, x, routes
    torch.cuda.empty_cache()
