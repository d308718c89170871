"""ms per movie and peak device memory above the inputs of the iterative sub-pixel patch alignment, next to what the
package offered for the same job before it, on the same 40 x 4092 x 5760 movie with 1024-px patches, in one process,
alternated, timed with device events after warm-up (medians):
  local     refine_local_motion(img, 1.0)                 (defaults: rigid refinement as the start, at most 10
                                                           iterations, threshold 0.01 px)
  fixed4    refine_local_motion(img, 1.0, max_iterations=4, convergence_threshold=0)    (no host reads in the loop)
  fixed1    the same with one iteration: per iteration = (fixed4 - fixed1) / 3
  passes    estimate_global_motion, then two passes of estimate_motion_cross_correlation_patches(deformation_field=
            previous): each pass normalises the movie and writes a warped fp32 copy of it
  raw_*     refine_local_motion_raw on the u8 counts of the same movie + a gain reference (no fp32 movie)
Prints one JSON line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_motion_correction_amd as mc  # noqa: E402

dev = torch.device("cuda:0")
t, h, w = (int(x) for x in os.environ.get("SHAPE", "40,4092,5760").split(","))
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))


def crop(base, sy, sx):
    """The texture at a drift of (sy, sx) px, bilinearly interpolated."""
    iy, ix, fy, fx = int(sy), int(sx), sy - int(sy), sx - int(sx)
    c = lambda a, b: base[16 + iy + a:16 + iy + a + h, 16 - ix - b:16 - ix - b + w]  # noqa: E731
    return (1 - fy) * (1 - fx) * c(0, 0) + fy * (1 - fx) * c(1, 0) + (1 - fy) * fx * c(0, 1) + fy * fx * c(1, 1)


def movie():
    """A smooth texture at a drift of a few pixels that is 0.8 px larger at the right edge than at the left (a blend of
    two rigidly drifted copies across x), + noise."""
    g = torch.Generator(device=dev).manual_seed(5)
    base = torch.randn((h + 32, w + 32), generator=g, device=dev)
    base = (base + torch.roll(base, 1, 0) + torch.roll(base, 1, 1) + torch.roll(base, (1, 1), (0, 1))) / 2
    u = torch.linspace(0, 1, w, device=dev)[None, :]
    img = torch.empty((t, h, w), dtype=torch.float32, device=dev)
    for f in range(t):
        sy, sx, loc = 5.4 * f / t, 3.7 * f / t, 0.8 * f / t
        img[f] = ((1 - u) * crop(base, sy, sx) + u * crop(base, sy + loc, sx + loc)
                  + 0.5 * torch.randn((h, w), generator=g, device=dev))
    return img


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (torch.cuda.max_memory_allocated() - base) / 2**30, out


def passes(img):
    field = mc.estimate_global_motion(img, 1.0)
    for _ in range(2):
        field, _ = mc.estimate_motion_cross_correlation_patches(img, 1.0, deformation_field=field)
    return field


img = movie()
gain = 1.0 + 0.1 * (2 * torch.rand((h, w), device=dev) - 1)
raw = ((20 * img + 110) / gain).round().clamp(0, 255).to(torch.uint8)
fixed = dict(convergence_threshold=0)
routes = {"local": lambda: mc.refine_local_motion(img, 1.0, return_history=True),
          "fixed4": lambda: mc.refine_local_motion(img, 1.0, max_iterations=4, **fixed),
          "fixed1": lambda: mc.refine_local_motion(img, 1.0, max_iterations=1, **fixed),
          "passes": lambda: passes(img),
          "raw_local": lambda: mc.refine_local_motion_raw(raw, gain, 1.0, return_history=True),
          "raw_fixed4": lambda: mc.refine_local_motion_raw(raw, gain, 1.0, max_iterations=4, **fixed),
          "raw_fixed1": lambda: mc.refine_local_motion_raw(raw, gain, 1.0, max_iterations=1, **fixed)}
ms, gib, hist = {k: [] for k in routes}, {}, {}
for i in range(warm + reps):
    for k, fn in routes.items():
        dt, peak, out = timed(fn)
        if i >= warm:
            ms[k].append(dt)
            gib[k] = round(peak, 3)
        if k in ("local", "raw_local"):
            hist[k] = [round(float(x), 5) for x in out[2]]
        del out
med = {k: round(statistics.median(v), 3) for k, v in ms.items()}
print(json.dumps({"frames": [t, h, w], "ms": med, "peak_gib_above_inputs": gib,
                  "per_iteration_ms": round((med["fixed4"] - med["fixed1"]) / 3, 3),
                  "raw_per_iteration_ms": round((med["raw_fixed4"] - med["raw_fixed1"]) / 3, 3),
                  "max_r": hist}), flush=True)
