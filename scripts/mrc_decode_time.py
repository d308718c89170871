"""ms and achieved GB/s (bytes read + written) of the MRC decode and of orient_raw next to the same operation written in
torch on the device, in one process, alternated, timed with device events after warm-up, medians of REPS (3):
  decode_101    decode_mrc_raw of a 40 x 4096^2 mode-101 movie     torch: stack((b & 15, b >> 4), -1)
  decode_6      decode_mrc_raw of a 40 x 4096^2 mode-6 movie       torch: bytes.view(int16).clone()  (a plain copy; the
                                                                     file's uint16 and the movie's int16 share their bits)
  decode_6_kernel  the same without decode_mrc_raw's check that no sample is 32768 or more (a reduction over the movie
                and a device-to-host read), which the torch expression does not make either
  orient_gain   orient_raw(gain, 1, "ud"), 4096^2 float32          torch: rot90(gain, 1, (-2, -1)).flip(-2).contiguous()
  orient_movie  orient_raw(movie, 1, "ud"), 40 x 4096^2 uint8      torch: the same expression
The data is on the device beforehand: the upload of the file is not what is compared.  Prints one JSON line, which
also quotes the plain stream-copy figure of profiles/r03_stream_copy_plain.txt ("copy_f4 U4 plain 4 blocks/CU")."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_motion_correction_amd as mc  # noqa: E402
from torch_motion_correction_amd import mrc  # noqa: E402

dev = torch.device("cuda:0")
T, H, W = (int(v) for v in os.environ.get("SHAPE", "40,4096,4096").split(","))
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))
STREAM_COPY_GBS = 4427.8  # profiles/r03_stream_copy_plain.txt: copy_f4 U4 plain 4 blocks/CU, avg

g = torch.Generator(device=dev).manual_seed(5)
header = torch.zeros(1024, dtype=torch.uint8, device=dev)
packed = torch.cat([header, torch.randint(0, 256, (T * H * (W // 2),), generator=g, device=dev, dtype=torch.uint8)])
words = torch.cat([header, torch.randint(0, 128, (T * H * W * 2,), generator=g, device=dev, dtype=torch.uint8)])
gain = torch.rand((H, W), generator=g, device=dev) + 0.5
movie = torch.randint(0, 16, (T, H, W), generator=g, device=dev, dtype=torch.uint8)
assert W % 2 == 0


def torch_101():
    b = packed[1024:].view(T, H, W // 2)
    return torch.stack((b & 15, b >> 4), -1).view(T, H, W)


def torch_6():
    return words[1024:].view(torch.int16).view(T, H, W).clone()


def torch_orient(x):
    return torch.rot90(x, 1, (-2, -1)).flip(-2).contiguous()


movie_bytes = T * H * W
routes = {
    "decode_101": (lambda: mc.decode_mrc_raw(packed, 1024, (T, H, W), 101), movie_bytes // 2 + movie_bytes),
    "decode_101_torch": (torch_101, movie_bytes // 2 + movie_bytes),
    "decode_6": (lambda: mc.decode_mrc_raw(words, 1024, (T, H, W), 6), 4 * movie_bytes),
    "decode_6_kernel": (lambda: mrc._decode(words, 1024, T, H, W, 6, False, False, False, dev), 4 * movie_bytes),
    "decode_6_torch": (torch_6, 4 * movie_bytes),
    "orient_gain": (lambda: mc.orient_raw(gain, 1, "ud"), 8 * H * W),
    "orient_gain_torch": (lambda: torch_orient(gain), 8 * H * W),
    "orient_movie": (lambda: mc.orient_raw(movie, 1, "ud"), 2 * movie_bytes),
    "orient_movie_torch": (lambda: torch_orient(movie), 2 * movie_bytes),
}
assert torch.equal(routes["decode_101"][0](), torch_101()) and torch.equal(routes["decode_6"][0](), torch_6())
assert torch.equal(routes["orient_gain"][0](), torch_orient(gain))
assert torch.equal(routes["orient_movie"][0](), torch_orient(movie))
for _ in range(warm):
    for fn, _ in routes.values():
        fn()
torch.cuda.synchronize()
ms = {k: [] for k in routes}
for _ in range(reps):
    for key, (fn, _) in routes.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms[key].append(a.elapsed_time(b))
        del out
res = {"shape": f"{T}x{H}x{W}"}
for k, v in ms.items():
    med = statistics.median(v)
    res[k] = {"median_ms": round(med, 3), "min_ms": round(min(v), 3), "gb_per_s": round(routes[k][1] / med / 1e6, 1)}
res["stream_copy_gb_per_s"] = STREAM_COPY_GBS
res["device"] = torch.cuda.get_device_name(dev)
print(json.dumps(res), flush=True)
