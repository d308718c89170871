"""ms of correct_magnification_distortion at (1.02, 0.98, 30 degrees) next to the same resampling written in torch on
the device and to a plain device copy of the same bytes, in one process, alternated, timed with device events after
warm-up, medians of REPS (3):
  sum_4096        one 4096 x 4096 fp32 sum
  stack_4096      a 40 x 4096 x 4096 fp32 stack (two chunks by the engine's workspace rule)
  stack_k3        a 40 x 4092 x 5760 fp32 stack
  *_torch         torch.nn.functional.grid_sample(bicubic, border, align_corners=True) over the same affine grid (fp32
                  coordinates: torch's own arithmetic; the grid is built beforehand and its read is part of the time)
  *_copy          Tensor.copy_ of the input into a buffer of the output's size: the floor, one read and one write of
                  4 bytes per pixel
The inputs are on the device beforehand and every route writes into a buffer allocated beforehand, but torch's
grid_sample, which allocates its result.  Before the timing the kernel's sum is compared with torch's (a loose check
of the convention at this size: torch's fp32 coordinates move a sample by up to ~1e-3 of a pixel).  Prints one JSON
line; gb_per_s counts 8 bytes per pixel."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_motion_correction_amd as mc  # noqa: E402
from torch_motion_correction_amd import magnification  # noqa: E402

dev = torch.device("cuda:0")
PARAMS = (1.02, 0.98, 30.0)
SHAPES = {"sum_4096": (1, 4096, 4096), "stack_4096": (40, 4096, 4096), "stack_k3": (40, 4092, 5760)}
if os.environ.get("SHAPES"):  # e.g. SHAPES=sum_4096,stack_4096
    SHAPES = {k: SHAPES[k] for k in os.environ["SHAPES"].split(",")}
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))
M = mc.magnification_distortion_matrix(*PARAMS)


def affine_grid(h, w):
    """grid_sample's normalised (x, y) grid of the rule's positions, fp32 (1, h, w, 2)."""
    dy = (torch.arange(h, dtype=torch.float64, device=dev) - h // 2)[:, None]
    dx = (torch.arange(w, dtype=torch.float64, device=dev) - w // 2)[None, :]
    py = (h // 2 + M[0, 0].item() * dy) + M[0, 1].item() * dx
    px = (w // 2 + M[1, 0].item() * dy) + M[1, 1].item() * dx
    return torch.stack([2 * px / (w - 1) - 1, 2 * py / (h - 1) - 1], dim=-1)[None].float(), \
        (py >= 0) & (py <= h - 1) & (px >= 0) & (px <= w - 1)


res = {"parameters": list(PARAMS)}
with torch.cuda.device(dev):
    for name, (t, h, w) in SHAPES.items():
        g = torch.Generator(device=dev).manual_seed(5)
        src = torch.randn((t, h, w), generator=g, device=dev) * 2 + 5
        out = torch.empty_like(src)
        grid, inside = affine_grid(h, w)

        def ours():
            return magnification._resample(src, M, 0.0, out=out)

        def by_torch():  # the frames as channels of one image: one grid for all of them
            return torch.nn.functional.grid_sample(src[None], grid, mode="bicubic", padding_mode="border",
                                                   align_corners=True)

        def copy():
            return out.copy_(src)

        routes = {name: ours, name + "_torch": by_torch, name + "_copy": copy}
        want = by_torch()[0, 0] * inside
        got = ours()[0]
        worst = float((got - want).abs().max())
        assert worst < 0.05, worst  # values of ~5 +- 2: a different convention would differ by several units
        del want, got
        for _ in range(warm):
            for fn in routes.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in routes}
        for _ in range(reps):
            for key, fn in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                r = fn()
                b.record()
                b.synchronize()
                ms[key].append(a.elapsed_time(b))
                del r
        for k, v in ms.items():
            med = statistics.median(v)
            res[k] = {"median_ms": round(med, 3), "min_ms": round(min(v), 3),
                      "gb_per_s": round(8 * t * h * w / med / 1e6, 1)}
        res[name]["max_abs_difference_to_torch"] = round(worst, 6)
        res[name]["x_copy"] = round(res[name]["median_ms"] / res[name + "_copy"]["median_ms"], 2)
        res[name]["x_torch"] = round(res[name]["median_ms"] / res[name + "_torch"]["median_ms"], 3)
        del src, out, grid, inside
        torch.cuda.empty_cache()
res["device"] = torch.cuda.get_device_name(dev)
print(json.dumps(res), flush=True)
