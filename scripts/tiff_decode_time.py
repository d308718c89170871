"""ms per movie of the TIFF LZW decode (decode_tiff_raw: mc_tiff_decode, one wavefront per strip over
csrc/tiff_lzw.h) on FRAMES (40) frames of H x W (4092 x 5760) Poisson u8 counts of mean MEAN (1.0), one process, timed
with device events after warm-up, medians of REPS (3), for strips of ROWS rows (11,2: 64 KB strips as libtiff cuts
them, and 2-row strips as SerialEM's):
  decode   the wrapper without its one device-to-host read of the per-strip byte counts, file already on the device
  copy     the bare device copy of the output's bytes, the decode's floor
  libtiff  where Pillow with libtiff is importable: its single-core decode of one such frame, times FRAMES
The strips come from tests/tiff_reference.py's encoder, which is pure Python: DISTINCT (64) different strips are
encoded and every strip of the movie is one of them in turn (strips may lie anywhere in `data`, so several may name
the same bytes).  The decode does the full movie's work -- every strip is parsed and its rows written -- while the
stream it reads is small and stays in cache; the stream is a quarter of the output's bytes.  Every distinct strip's
rows are compared with the counts they were made from before anything is timed.  There is no earlier implementation
to compare against: the numbers are those of a new stage.  Prints one JSON line."""
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
mean, distinct = float(os.environ.get("MEAN", "1.0")), int(os.environ.get("DISTINCT", "64"))
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


res = {"frames": frames, "shape": f"{h}x{w}", "mean": mean, "output_mb": round(frames * h * w / 1e6, 1)}
rng = np.random.default_rng(1)
for rps in rows:
    spf = (h + rps - 1) // rps
    last = h - (spf - 1) * rps
    counts = rng.poisson(mean, (distinct, rps, w)).astype(np.uint8)
    full = [tr.encode_strip(c.tobytes()) for c in counts]
    short = [tr.encode_strip(c[:last].tobytes()) for c in counts] if last != rps else full
    blob, at = bytearray(), {}
    for kind, group in (("full", full), ("short", short)):
        for i, s in enumerate(group):
            at[kind, i] = (len(blob), len(s))
            blob += s
    flat_o, flat_n = [], []
    for s in range(frames * spf):
        o, n = at["short" if s % spf == spf - 1 else "full", s % distinct]
        flat_o.append(o)
        flat_n.append(n)
    data = torch.frombuffer(blob, dtype=torch.uint8).to(dev)
    args = (data, flat_o, flat_n, frames, spf, h, w, rps, 5, dev)
    out, produced = tiff._decode_strips(*args)
    want = tiff._expected(spf, h, w, rps)
    assert produced.cpu().tolist() == want * frames
    movie = out.view(frames, h, w)
    for s in list(range(min(distinct, spf))) + [spf - 1, (frames - 1) * spf + spf - 1]:
        k, f = s % spf, s // spf
        got = movie[f, k * rps:k * rps + (last if k == spf - 1 else rps)].cpu()
        assert torch.equal(got, torch.from_numpy(counts[s % distinct][:got.shape[0]])), (rps, s)
    codes = []
    tr.decode_strip(full[0], rps * w, codes)
    del out, movie
    res[f"rows{rps}"] = {"strips": frames * spf, "strip_kb": round(rps * w / 1e3, 1), "codes_per_strip": len(codes),
                         "stream_over_output": round(sum(flat_n) / (frames * h * w), 3),
                         "decode": timed(lambda: tiff._decode_strips(*args))}
out = tiff._decode_strips(*args)[0]  # a decoded movie: memory that has been written
res["copy"] = timed(lambda: out.clone())
try:
    from PIL import Image, features

    if features.check("libtiff"):
        buf = io.BytesIO()
        Image.fromarray(rng.poisson(mean, (h, w)).astype(np.uint8)).save(buf, format="TIFF", compression="tiff_lzw")
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            Image.open(io.BytesIO(buf.getvalue())).load()
            t.append(time.perf_counter() - t0)
        res["libtiff_one_core_ms"] = round(statistics.median(t) * 1e3 * frames, 1)
except ImportError:
    pass
res["device"] = torch.cuda.get_device_name(dev)
print(json.dumps(res), flush=True)
