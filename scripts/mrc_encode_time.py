"""ms and achieved GB/s (bytes read + written) of the MRC encode next to the same bytes moved by torch.clone and to the
same operation written in torch on the device, in one process, alternated, timed with device events after warm-up,
medians of REPS (3):
  encode_101    encode_mrc_raw of a 40 x 4096^2 uint8 movie to mode 101    torch: a[..., 0::2] | a[..., 1::2] << 4, then
                                                                           min, max, sum and sum of squares (int64)
  encode_0      the same movie to mode 0                                   torch: clone, then the four reductions
  encode_1      encode_mrc_raw of a 40 x 4096^2 int16 movie to mode 1      torch: clone, then the four reductions
  *_clone       torch.clone of a tensor of the payload's size: the payload's bytes read once and written once (modes 0
                and 1: exactly the bytes the encode moves; mode 101: the encode reads twice as many as it writes)
encode_mrc_raw's time includes the device-to-host read of its statistics table.  The movie is on the device
beforehand.  Prints one JSON line, which also quotes the decoder's time for the mode-101
payload ("MRC decode and gain orientation") and the plain stream-copy figure of
profiles/r03_stream_copy_plain.txt ("copy_f4 U4 plain 4 blocks/CU")."""
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
DECODE_101_MS = 0.21  # decode_mrc_raw of the same mode-101 payload
assert W % 2 == 0

g = torch.Generator(device=dev).manual_seed(5)
counts = torch.randint(0, 16, (T, H, W), generator=g, device=dev, dtype=torch.uint8)
words = torch.randint(-32768, 32768, (T, H, W), generator=g, device=dev, dtype=torch.int16)
half = torch.empty(T * H * W // 2, dtype=torch.uint8, device=dev)


def reductions(a):
    wide = a.view(-1, 1 << 20)  # int64 sums of blocks, not an int64 copy of the movie
    return a.min(), a.max(), wide.sum(1, dtype=torch.int64).sum(), (wide.to(torch.int32) ** 2).sum(1, dtype=torch.int64).sum()


def torch_101():
    return counts[..., 0::2] | counts[..., 1::2] << 4, reductions(counts)


def clones(*tensors):
    return [x.clone() for x in tensors]


n = T * H * W
routes = {
    "encode_101": (lambda: mc.encode_mrc_raw(counts, mode=101), n + n // 2),
    "encode_101_torch": (torch_101, n + n // 2),
    "encode_101_clone": (lambda: clones(half), n),  # reads n / 2 and writes n / 2: fewer bytes than the encode moves
    "encode_0": (lambda: mc.encode_mrc_raw(counts, mode=0), 2 * n),
    "encode_0_torch": (lambda: (counts.clone(), reductions(counts)), 2 * n),
    "encode_0_clone": (lambda: clones(counts), 2 * n),
    "encode_1": (lambda: mc.encode_mrc_raw(words, mode=1), 4 * n),
    "encode_1_torch": (lambda: (words.clone(), reductions(words)), 4 * n),
    "encode_1_clone": (lambda: clones(words), 4 * n),
}
enc, table = mc.encode_mrc_raw(counts, mode=101, return_statistics=True)
packed, (lo, hi, total, squares) = torch_101()
assert torch.equal(enc.data.view(T, H, W // 2), packed) and torch.equal(enc.decode(), counts)
assert (int(table[:, 0].min()), int(table[:, 1].max()), int(table[:, 2].sum()), int(table[:, 3].sum())) == \
    (int(lo), int(hi), int(total), int(squares))
enc, table = mc.encode_mrc_raw(words, mode=1, return_statistics=True)
lo, hi, total, squares = reductions(words)
assert torch.equal(enc.data.view(torch.int16).view(T, H, W), words)
assert (int(table[:, 0].min()), int(table[:, 1].max()), int(table[:, 2].sum()), int(table[:, 3].sum())) == \
    (int(lo), int(hi), int(total), int(squares))
del enc, packed
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
res["decode_101_ms_recorded"] = DECODE_101_MS
res["stream_copy_gb_per_s"] = STREAM_COPY_GBS
res["device"] = torch.cuda.get_device_name(dev)
print(json.dumps(res), flush=True)
