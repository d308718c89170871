"""ms per movie of the detector-defect fill (fill_defects_raw: the movie's copy + mc_raw_fill_defects on the copy)
against the bare copy of the same movie (movie.clone()) at the same commit, in one process, alternated, timed with
device events after warm-up, medians of REPS (3):
  fill      fill_defects_raw(movie, plan)                  out of place: copy + kernel
  in_place  fill_defects_raw(movie, plan, in_place=True)   the kernel alone (refilling a filled movie: same work)
  copy      movie.clone()
  plan      DefectFill(defect_map)                         once per session: nonzero + mc_defect_donors + one read
Size: 4k (40 x 4096^2 u8), or SIZES=4k,c5 (c5: 60 x 8184 x 11520); DTYPE=int16 / float32 for other element sizes.
The defect map is a detector's: two dead columns, one dead row, a 6 x 6 block and 2000 scattered pixels.  The filled
movie is compared first: every defect of three frames holds one of its donors' values, everything else is the movie.
Prints one JSON line per size."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch_motion_correction_amd as mc  # noqa: E402

dev = torch.device("cuda:0")
SIZES = {"4k": (40, 4096, 4096), "c5": (60, 8184, 11520)}
warm, reps = int(os.environ.get("WARMUP", "1")), int(os.environ.get("REPS", "3"))
dtype = {"uint8": torch.uint8, "int16": torch.int16, "float32": torch.float32}[os.environ.get("DTYPE", "uint8")]


def movie(t, h, w):
    g = torch.Generator(device=dev).manual_seed(5)
    raw = torch.empty((t, h, w), dtype=dtype, device=dev)
    for f in range(t):  # Poisson-like counts, a frame at a time: nothing movie-sized besides the movie
        v = 20.0 + 4.5 * torch.randn((h, w), generator=g, device=dev)
        raw[f] = v.round().clamp(0, 255).to(dtype)
        del v
    return raw


def detector_map(h, w):
    g = torch.Generator().manual_seed(11)
    m = torch.zeros((h, w), dtype=torch.bool)
    m[:, w // 3] = m[:, w // 3 + 1] = True
    m[h // 2, :] = True
    m[100:106, 200:206] = True
    m.view(-1)[torch.randint(0, h * w, (2000,), generator=g)] = True
    return m


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    del out
    return a.elapsed_time(b)


for name in os.environ.get("SIZES", "4k").split(","):
    t, h, w = SIZES[name]
    raw = movie(t, h, w)
    dmap = detector_map(h, w).to(dev)
    plan = mc.DefectFill(dmap)
    out = mc.fill_defects_raw(raw, plan, seed=1)
    for f in (0, t // 2, t - 1):
        a, b = raw[f].view(-1), out[f].view(-1)
        assert torch.equal(b[~dmap.view(-1)], a[~dmap.view(-1)])
        donors = a[plan.donors.clamp(min=0).long()]  # (n, 8 reach) donor values; unused slots masked below
        hit = (donors == b[plan.pixels.long()][:, None]) & (plan.donors >= 0)
        assert bool(hit.any(dim=1).all())
    work = out  # the in-place route refills this copy
    del out
    routes = {"fill": lambda: mc.fill_defects_raw(raw, plan, seed=1),
              "in_place": lambda: mc.fill_defects_raw(work, plan, seed=1, in_place=True),
              "copy": lambda: raw.clone(),
              "plan": lambda: mc.DefectFill(dmap)}
    for _ in range(warm):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for key, fn in routes.items():
            ms[key].append(timed(fn))
    nbytes = raw.numel() * raw.element_size()
    res = {"size": f"{t}x{h}x{w}", "dtype": str(dtype), "movie_gb": round(nbytes / 1e9, 3), "defects": plan.n}
    for k, v in ms.items():
        res[k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3)}
    res["fill_over_copy"] = round(statistics.median(ms["fill"]) / statistics.median(ms["copy"]), 3)
    res["device"] = torch.cuda.get_device_name(dev)
    print(json.dumps(res), flush=True)
    del raw, work, plan, routes
    torch.cuda.empty_cache()
