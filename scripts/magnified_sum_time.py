"""ms per movie and peak device memory above the inputs of the aligned, magnification-corrected sum of a 40 x 4096^2
movie at (1.02, 0.98, 30 degrees) with fractional rigid shifts, by the one-pass route and by the two-step routes that
give the same image with two interpolations, in one process, alternated, timed with device events after warm-up,
medians of REPS (3):
  fp32       motion_correct_sum_magnified(stack, field, ps, ...)               one interpolation
  fp32_two   motion_correct_sum(stack, field, ps) -> correct_magnification_distortion(sum, ...)
  raw        motion_correct_sum_magnified_raw(movie u8, gain, field, ps, ...)  one interpolation, no fp32 movie
  raw_two    motion_correct_sum_raw(movie, gain, field, ps) -> correct_magnification_distortion(sum, ...)
  raw_cond   condition_movie(movie, gain) -> motion_correct_sum_magnified(fp32 movie, ...)
The inputs are on the device beforehand.  Before the timing the one-pass and the two-step sums are compared (a loose
check: they differ by the second interpolation's smoothing and at the border).  ROUTES=fp32,raw,... picks routes.
Prints one JSON line."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_motion_correction_amd as mc  # noqa: E402

dev = torch.device("cuda:0")
PARAMS = (1.02, 0.98, 30.0)
PS = 0.83
T, H, W = (int(v) for v in os.environ.get("SHAPE", "40,4096,4096").split(","))
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))


def movie():
    g = torch.Generator(device=dev).manual_seed(5)
    base = torch.rand((H + 32, W + 32), generator=g, device=dev) * 40 + 10
    raw = torch.empty((T, H, W), dtype=torch.uint8, device=dev)
    for f in range(T):
        dy, dx = (f * 3) // T, (f * 5) // T
        noise = torch.randn((H, W), generator=g, device=dev) * 4
        raw[f] = (base[16 + dy:16 + dy + H, 16 - dx:16 - dx + W] + noise).round().clamp(0, 255).to(torch.uint8)
        del noise
    gain = (1.0 + 0.1 * torch.randn((H, W), generator=g, device=dev)).clamp(0.5, 1.5)
    return raw, gain


# a rigid drift of a few pixels with sub-pixel parts, (2, t, 1, 1) Angstrom
tt = torch.linspace(-1, 1, T)
field = (torch.stack([2.7 * tt, -3.2 * tt]) * PS)[:, :, None, None].contiguous()

with torch.cuda.device(dev):
    raw, gain = movie()
    stack = mc.condition_movie(raw, gain)
    field_dev = field.to(dev)  # the existing routes evaluate the field on the device, the new ones on the host
    routes = {
        "fp32": lambda: mc.motion_correct_sum_magnified(stack, field, PS, *PARAMS),
        "fp32_two": lambda: mc.correct_magnification_distortion(mc.motion_correct_sum(stack, field_dev, PS), *PARAMS),
        "raw": lambda: mc.motion_correct_sum_magnified_raw(raw, gain, field, PS, *PARAMS),
        "raw_two": lambda: mc.correct_magnification_distortion(mc.motion_correct_sum_raw(raw, gain, field_dev, PS), *PARAMS),
        "raw_cond": lambda: mc.motion_correct_sum_magnified(mc.condition_movie(raw, gain), field, PS, *PARAMS),
    }
    if os.environ.get("ROUTES"):
        routes = {k: routes[k] for k in os.environ["ROUTES"].split(",")}
    res = {"size": f"{T}x{H}x{W}", "parameters": list(PARAMS), "pixel_spacing": PS, "reps": reps, "warmup": warm,
           "input_gb": {"fp32": round(stack.numel() * 4 / 1e9, 2), "raw": round((raw.numel() + gain.numel() * 4) / 1e9, 2)}}
    # the convention, on a SMOOTH 3 x 512 x 512 movie (waves of 40 px and more: a second bicubic pass changes such an
    # image by little, while a shift of the wrong sign or axis moves it by pixels): one pass against two steps
    yy, xx = torch.meshgrid(torch.arange(512.0, device=dev), torch.arange(512.0, device=dev), indexing="ij")
    smooth = torch.stack([torch.sin(yy / 7 + k) * torch.cos(xx / 9 - k) + torch.sin((yy + 2 * xx) / 23) for k in range(3)])
    sf = (torch.tensor([[5.3, -7.6, 2.2], [-4.1, 6.7, -9.4]]) * PS)[:, :, None, None].contiguous()
    one = mc.motion_correct_sum_magnified(smooth, sf, PS, *PARAMS)
    two = mc.correct_magnification_distortion(mc.motion_correct_sum(smooth, sf.to(dev), PS), *PARAMS)
    flipped = mc.motion_correct_sum_magnified(smooth, -sf, PS, *PARAMS)
    inner = (slice(32, -32), slice(32, -32))
    worst, wrong = float((one - two)[inner].abs().max()), float((flipped - two)[inner].abs().max())
    res["smooth_check"] = {"one_pass_minus_two_step_max_abs": round(worst, 5), "with_the_shifts_negated": round(wrong, 3),
                           "same_convention": worst < 0.1 < 1.0 < wrong}  # three waves of amplitude ~2 a frame, Keys cubic twice
    del yy, xx, smooth, one, two, flipped
    if "fp32" in routes and "fp32_two" in routes:  # on the timed movie, whose texture is white noise
        one, two = routes["fp32"](), routes["fp32_two"]()
        inner = (slice(256, H - 256), slice(256, W - 256))
        res["one_pass_minus_two_step"] = {"max_abs": round(float((one - two)[inner].abs().max()), 4),
                                          "rms": round(float((one - two)[inner].square().mean().sqrt()), 5),
                                          "rms_of_sum": round(float(one[inner].square().mean().sqrt()), 3)}
        del one, two
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
