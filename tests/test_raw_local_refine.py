"""Iterative sub-pixel patch alignment straight from raw u8 / i16 movies (refine_local_motion_raw) against
refine_local_motion on condition_movie's fp32 movie: the same field within the fp32 rounding of the conditioning,
without a conditioned movie; every case the fused route does not take runs exactly the conditioned route."""

import numpy as np
import pytest
import torch

import local_refine_reference as lr
from torch_motion_correction_amd import engine

pytestmark = pytest.mark.gpu

SHAPE, P, ITER = (6, 1536, 2048), 1024, 4


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


@pytest.fixture(scope="module")
def movie():
    """Planted local motion: fractional rigid drift plus a local part of 1 px (x) across the frame."""
    t = SHAPE[0]
    f = np.arange(t) - t // 2
    rigid = np.stack([np.linspace(-3.3, 4.6, t), np.linspace(2.7, -1.9, t)], axis=1)
    slope = np.stack([0.4 * np.sin(0.8 * f), -1.0 * f / (t // 2)], axis=1)
    return lr.planted_local_movie(*SHAPE, rigid, slope, noise=0.25, seed=21)[0]


def raw_movie(movie, dev, dtype, hot=False):
    """Detector counts of the movie and a gain reference of 1 +- 0.1; with `hot`, a few hot pixels per frame."""
    t, h, w = movie.shape
    g = torch.Generator().manual_seed(5)
    gain = 1.0 + 0.1 * (2 * torch.rand(h, w, generator=g) - 1)
    if dtype == torch.uint8:
        raw = ((20 * movie + 110) / gain).round().clamp(0, 255).to(dtype)
    else:
        raw = ((300 * movie - 200) / gain).round().clamp(-32768, 32767).to(dtype)
    if hot:
        hi = 255 if dtype == torch.uint8 else 30000
        for f in range(t):
            ys, xs = torch.randint(0, h, (6,), generator=g), torch.randint(0, w, (6,), generator=g)
            raw[f, ys, xs] = hi
            gain[ys, xs] = 1.0
    return raw.to(dev), gain.to(dev)


def range_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.max() - b.min()), 1e-30))


def refuse(*a, **k):
    raise AssertionError("the fused route conditioned the movie")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
def test_raw_route_matches_the_conditioned_route(mc, dev, movie, dtype, monkeypatch):
    raw, gain = raw_movie(movie, dev, dtype)
    img = mc.condition_movie(raw, gain)
    want, want_centres, want_hist = mc.refine_local_motion(img, 1.0, P, max_iterations=ITER, convergence_threshold=0,
                                                           return_history=True)
    del img
    monkeypatch.setattr(engine, "condition_movie", refuse)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got, centres, hist = mc.refine_local_motion_raw(raw, gain, 1.0, P, max_iterations=ITER, convergence_threshold=0,
                                                    return_history=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    monkeypatch.undo()
    err = range_err(got, want)
    t, h, w = SHAPE
    print(f"{dtype}: raw against conditioned field {err:.3e} of its range, history "
          f"{float((hist - want_hist).abs().max()):.3e} px, peak {peak / 2**20:.1f} MiB above the inputs "
          f"(one fp32 movie: {t * h * w * 4 / 2**20:.1f} MiB)")
    assert tuple(got.shape) == (2, t, 1, 2) and len(hist) == ITER and torch.equal(centres, want_centres)
    assert err <= 1e-5, err  # the bound of the raw-against-conditioned tests (tests/test_global_refine.py)
    assert float(got[:, t // 2].abs().max()) == 0.0 and float(got.abs().max()) > 1.0
    assert peak < t * h * w * 4, peak  # never as much as one fp32 movie
    # the one-line recipe: the field feeds the raw sums, which equal the conditioned route's for the same field
    s_raw = mc.motion_correct_sum_raw(raw, gain, got, 1.0)
    s_img = mc.motion_correct_sum(mc.condition_movie(raw, gain), got, 1.0)
    assert range_err(s_raw, s_img) <= 1e-5, range_err(s_raw, s_img)


def test_start_field_from_the_raw_global_refinement(mc, dev, movie):
    """The global-then-local flow from raw bytes: the default start is refine_global_motion_raw's field."""
    raw, gain = raw_movie(movie, dev, torch.uint8)
    rigid = mc.refine_global_motion_raw(raw, gain, 1.0)
    a = mc.refine_local_motion_raw(raw, gain, 1.0, P, deformation_field=rigid, max_iterations=2, convergence_threshold=0)
    b = mc.refine_local_motion_raw(raw, gain, 1.0, P, max_iterations=2, convergence_threshold=0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("kw", [dict(hot_pixel_threshold=10.0), dict(patch_sidelength=512)])
def test_other_cases_take_exactly_the_conditioned_route(mc, dev, movie, kw):
    hot = kw.get("hot_pixel_threshold")
    raw, gain = raw_movie(movie[:4], dev, torch.uint8, hot=hot is not None)
    p = kw.get("patch_sidelength", P)
    got = mc.refine_local_motion_raw(raw, gain, 1.0, p, max_iterations=2, convergence_threshold=0,
                                     hot_pixel_threshold=hot)
    img = mc.condition_movie(raw, gain, hot_pixel_threshold=hot)
    want = mc.refine_local_motion(img, 1.0, p, max_iterations=2, convergence_threshold=0)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert float(got[0].abs().max()) > 1.0
    # and the engine refuses them rather than falling back silently
    rm = engine.RawMovie(raw, gain, hot_pixel_threshold=hot)
    with pytest.raises(engine._lib.McorrUnsupported):
        engine.local_shifts_raw_refined(rm, 1.0, p, None, 2, 500.0, (300, 10), 2, 0.0)
