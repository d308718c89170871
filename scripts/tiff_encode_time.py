"""ms per movie of the TIFF LZW encode (encode_tiff_raw: mc_tiff_encode, one wavefront per strip over
csrc/tiff_lzw_encode.h, then mc_tiff_pack) on FRAMES (40) frames of H x W (4092 x 5760) Poisson u8 counts of mean MEAN
(1.0), one process, timed with device events after warm-up, medians of REPS (3), for strips of ROWS rows (11,2: 64 KB
strips as libtiff cuts them, and 2-row strips as SerialEM's):
  encode   mc_tiff_encode alone: every strip into its slot, the per-strip sizes on the device
  pack     the device scan of the sizes and mc_tiff_pack: the slots' bytes into one payload
  whole    encode_tiff_raw, its one device-to-host read of the sizes included (host wall time)
  decode   the decoder (mc_tiff_decode) on the strips just made
  copy     the bare device copy of the input's bytes, the encode's floor
  libtiff  where Pillow with libtiff is importable: its single-core encode of one such frame, times FRAMES
Before anything is timed, a handful of strips are compared with tests/tiff_reference.py's encoder byte for byte and
the decoded movie with the input.  There is no earlier implementation to compare against: the numbers are those of a
new stage.  Prints one JSON line."""
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tiff_reference as tr  # noqa: E402
from torch_motion_correction_amd import tiff  # noqa: E402

dev = torch.device("cuda:0")
frames, h, w = int(os.environ.get("FRAMES", "40")), int(os.environ.get("H", "4092")), int(os.environ.get("W", "5760"))
mean = float(os.environ.get("MEAN", "1.0"))
rows = [int(r) for r in os.environ.get("ROWS", "11,2").split(",")]
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))


def timed(fn):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
        del out
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3)}


def wall(fn):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        del out
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3)}


res = {"frames": frames, "shape": f"{h}x{w}", "mean": mean, "input_mb": round(frames * h * w / 1e6, 1)}
gen = torch.Generator(device=dev).manual_seed(1)
movie = torch.poisson(torch.full((frames, h, w), mean, device=dev), generator=gen).clamp_(max=255).to(torch.uint8)
src = movie.view(-1)
for rps in rows:
    spf = (h + rps - 1) // rps
    enc = tiff.encode_tiff_raw(movie, rows_per_strip=rps)
    assert torch.equal(enc.decode(), movie)
    data = enc.data.cpu().numpy()
    for f, k in ((0, 0), (0, spf - 1), (frames - 1, spf // 2)):
        strip = movie[f, k * rps:(k + 1) * rps].cpu().numpy().tobytes()
        o, n = enc.offsets[f][k], enc.nbytes[f][k]
        assert bytes(data[o:o + n]) == tr.encode_strip(strip), (rps, f, k)
    slots, slot, produced = tiff._encode_strips(src, frames, spf, h, w, rps, dev)
    total = int(produced.sum())
    flat_o = [o for fo in enc.offsets for o in fo]
    flat_n = [n for fn in enc.nbytes for n in fn]
    res[f"rows{rps}"] = {
        "strips": frames * spf, "strip_kb": round(rps * w / 1e3, 1), "slot_kb": round(slot / 1e3, 1),
        "payload_over_input": round(total / (frames * h * w), 4),
        "encode": timed(lambda: tiff._encode_strips(src, frames, spf, h, w, rps, dev, slots=slots)),
        "pack": timed(lambda: tiff._pack_strips(slots, slot, produced, total, dev)),
        "whole": wall(lambda: tiff.encode_tiff_raw(movie, rows_per_strip=rps)),
        "decode": timed(lambda: tiff._decode_strips(enc.data, flat_o, flat_n, frames, spf, h, w, rps, 5, dev))}
    del slots, enc
res["copy"] = timed(lambda: movie.clone())
try:
    from PIL import Image, features

    if features.check("libtiff"):
        frame = movie[0].cpu().numpy()
        t = []
        for _ in range(reps):
            buf = io.BytesIO()
            t0 = time.perf_counter()
            Image.fromarray(frame).save(buf, format="TIFF", compression="tiff_lzw")
            t.append(time.perf_counter() - t0)
        res["libtiff_one_core_ms"] = round(statistics.median(t) * 1e3 * frames, 1)
except ImportError:
    pass
res["device"] = torch.cuda.get_device_name(dev)
print(json.dumps(res), flush=True)
