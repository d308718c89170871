"""ms per movie of three routes for one 40 x 4096^2 u8 movie with a gain reference, in one process, alternated,
timed with device events after warm-up:
  fused       motion_correct_raw(raw, gain)                                  (no hot-pixel step)
  fused_hot   motion_correct_raw(raw, gain, hot_pixel_threshold=10)          (sparse corrections)
  cond_hot    condition_movie(raw, gain, hot_pixel_threshold=10) + estimate_global_motion + motion_correct_sum
The movie carries a few hundred hot pixels per frame.  Prints one JSON line (median and min per route)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_motion_correction_amd as mc  # noqa: E402

dev = torch.device("cuda:0")
t, h, w = 40, 4096, 4096
g = torch.Generator(device=dev).manual_seed(5)
raw = (torch.rand((t, h, w), generator=g, device=dev) * 40 + 10).round().to(torch.uint8)
gain = (1.0 + 0.1 * torch.randn((h, w), generator=g, device=dev)).clamp(0.5, 1.5)
for f in range(t):
    ys = torch.randint(0, h, (300,), generator=g, device=dev)
    xs = torch.randint(0, w, (300,), generator=g, device=dev)
    raw[f, ys, xs] = 255

routes = {
    "fused": lambda: mc.motion_correct_raw(raw, gain, 1.0),
    "fused_hot": lambda: mc.motion_correct_raw(raw, gain, 1.0, hot_pixel_threshold=10.0),
    "cond_hot": lambda: mc.motion_correct_sum(img := mc.condition_movie(raw, gain, hot_pixel_threshold=10.0),
                                              mc.estimate_global_motion(img, 1.0), 1.0),
}
warm, reps = int(os.environ.get("WARMUP", "3")), int(os.environ.get("REPS", "10"))
for _ in range(warm):
    for fn in routes.values():
        fn()
torch.cuda.synchronize()
ms = {k: [] for k in routes}
for _ in range(reps):
    for name, fn in routes.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms[name].append(a.elapsed_time(b))
out = {k: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3)} for k, v in ms.items()}
out["hot_minus_plain_ms"] = round(out["fused_hot"]["median_ms"] - out["fused"]["median_ms"], 3)
out["device"] = torch.cuda.get_device_name(dev)
print(json.dumps(out))
