"""ms per movie of the EER render (render_eer_raw: mc_eer_render, three passes over csrc/eer.h) on a synthetic stream
of FRAMES (256) frames of SIDE^2 (4096^2) pixels, DENSITY (0.02) events per pixel and frame, GROUP (8), one process,
timed with device events after warm-up, medians of REPS (3):
  render   the library's segment size (SEGMENTS=64,128,256 times each of those instead), stream already on the device
  zero     the bare zero_() of the output
  copy     a device copy of the stream's bytes
The last two are the render's floor: it has to clear the output and to read the stream once.  The frames come from
tests/eer_reference.py's encoder (gaps drawn geometrically: the same distribution as one Bernoulli draw per pixel);
for each segment size the first frame is compared with the positions it was drawn from, every frame's final n with
h * w and the movie's total with the event counts before anything is timed.  `render` is the wrapper without its one
device-to-host read of the final pixel counts.  There is no earlier
implementation to compare against: the numbers are those of a new stage.  Prints one JSON line."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eer_reference as er  # noqa: E402
from torch_motion_correction_amd import eer  # noqa: E402

dev = torch.device("cuda:0")
frames, side = int(os.environ.get("FRAMES", "256")), int(os.environ.get("SIDE", "4096"))
density, group = float(os.environ.get("DENSITY", "0.02")), int(os.environ.get("GROUP", "8"))
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))
segments = [int(s) for s in os.environ.get("SEGMENTS", str(eer.SEGMENT_BYTES)).split(",")]
n = side * side

rng = np.random.default_rng(1)
strips, first = [], None
for _ in range(frames):
    pos = np.cumsum(rng.geometric(density, size=int(n * density * 1.2) + 64)) - 1
    pos = pos[pos < n]
    first = pos if first is None else first
    strips.append(er.encode_frame(pos, rng.integers(0, 16, size=pos.size), n))
nbytes = [len(s) for s in strips]
offsets = [int(o) for o in np.cumsum([0] + nbytes[:-1])]
data = torch.frombuffer(bytearray(b"".join(strips)), dtype=torch.uint8).to(dev)
events = 0


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


res = {"frames": frames, "shape": f"{side}x{side}", "density": density, "group": group,
       "stream_mb": round(data.numel() / 1e6, 1), "output_mb": round(frames // group * n / 1e6, 1)}
want = torch.zeros(n, dtype=torch.uint8)
want[torch.from_numpy(first)] = 1  # the first frame as it was drawn
want = want.reshape(1, side, side)
for seg in segments:
    movie, final_n, counts = eer._render(data, offsets, nbytes, side, side, group, 1, dev, segment_bytes=seg)
    assert bool((final_n == n).all())
    one = eer._render(data, offsets[:1], nbytes[:1], side, side, 1, 1, dev, segment_bytes=seg)[0]
    assert torch.equal(one.cpu(), want), seg
    assert int(movie.sum(dtype=torch.int64)) == int(counts[:frames // group * group].sum())
    events = int(counts.sum())
    del movie, one
    res[f"render_S{seg}"] = timed(lambda: eer._render(data, offsets, nbytes, side, side, group, 1, dev,
                                                      segment_bytes=seg))
out = torch.empty((frames // group, side, side), dtype=torch.uint8, device=dev)
res["zero"] = timed(lambda: out.zero_())
res["copy"] = timed(lambda: data.clone())
res["events"] = events
res["device"] = torch.cuda.get_device_name(dev)
print(json.dumps(res), flush=True)
