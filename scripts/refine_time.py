"""ms per movie of the iterative sub-pixel whole-frame alignment next to the integer estimate it starts from, on the
same fp32 movie, in one process, alternated, timed with device events after warm-up (medians):
  refine    refine_global_motion(img, 1.0)                    (defaults: at most 10 iterations, threshold 0.01 px)
  fixed     refine_global_motion(img, 1.0, max_iterations=4, convergence_threshold=0)   (no host reads in the loop)
  estimate  estimate_global_motion(img, 1.0)                   (the yardstick: the whole integer estimate)
Sizes: 4k (40 x 4096^2) and c3 (40 x 4092 x 5760), or SIZES=4k,c3.  Prints one JSON line per size with the iterations
used and the cost per iteration, (fixed - estimate) / 4."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_motion_correction_amd as mc  # noqa: E402

dev = torch.device("cuda:0")
SIZES = {"4k": (40, 4096, 4096), "c3": (40, 4092, 5760)}
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))


def movie(t, h, w):
    """A smooth texture cropped at a drift of a few pixels, bilinearly interpolated to sub-pixel offsets, + noise."""
    g = torch.Generator(device=dev).manual_seed(5)
    base = torch.randn((h + 32, w + 32), generator=g, device=dev)
    base = (base + torch.roll(base, 1, 0) + torch.roll(base, 1, 1) + torch.roll(base, (1, 1), (0, 1))) / 2
    img = torch.empty((t, h, w), dtype=torch.float32, device=dev)
    for f in range(t):
        sy, sx = 5.4 * f / t, 3.7 * f / t
        iy, ix, fy, fx = int(sy), int(sx), sy - int(sy), sx - int(sx)
        c = lambda a, b: base[16 + iy + a:16 + iy + a + h, 16 - ix - b:16 - ix - b + w]  # noqa: E731
        img[f] = ((1 - fy) * (1 - fx) * c(0, 0) + fy * (1 - fx) * c(1, 0) + (1 - fy) * fx * c(0, 1) + fy * fx * c(1, 1)
                  + 0.5 * torch.randn((h, w), generator=g, device=dev))
    return img


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


for name in os.environ.get("SIZES", "4k,c3").split(","):
    t, h, w = SIZES[name]
    img = movie(t, h, w)
    routes = {"refine": lambda: mc.refine_global_motion(img, 1.0, return_history=True),
              "fixed": lambda: mc.refine_global_motion(img, 1.0, max_iterations=4, convergence_threshold=0),
              "estimate": lambda: mc.estimate_global_motion(img, 1.0)}
    ms = {k: [] for k in routes}
    hist = None
    for i in range(warm + reps):
        for k, fn in routes.items():
            dt, out = timed(fn)
            if i >= warm:
                ms[k].append(dt)
            if k == "refine":
                hist = out[1]
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"size": name, "frames": [t, h, w], "refine_ms": round(med["refine"], 3),
                      "fixed4_ms": round(med["fixed"], 3), "estimate_ms": round(med["estimate"], 3),
                      "per_iteration_ms": round((med["fixed"] - med["estimate"]) / 4, 3),
                      "iterations_used": len(hist), "max_r": [round(float(x), 5) for x in hist]}), flush=True)
    del img
