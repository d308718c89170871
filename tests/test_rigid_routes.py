"""The rigid warp's routes agree bit for bit at pixel spacings != 1, for both spline grids, short movies and any
reference frame: the movie pipeline's tail (rigid_tail), the generic route (image_shifts_to_deformation_field ->
frame_lattices -> rigid_tables), the per-call API functions and the raw-movie routes all apply the canonical
per-frame shift fp32(L) / fp32(ps) (tests/rigid_reference.py).  Frames are compared with a float64 resampler of
the reference's sampling rule with no knife-edge mask: a shift one ulp towards the border zeroes a whole row or
column that the reference keeps, and the pattern of exact zeros must match."""

import numpy as np
import pytest
import torch

from kernel_harness import drifting_raw_movie, mc, rel_err  # noqa: F401
from rigid_reference import (FRAME_SPACINGS, LARGE_SHIFTS, PIPELINE_SPACINGS, RAW_SPACINGS, SMALL_SHIFTS,
                             TABLE_SPACINGS, assert_frames as _assert_frames, canonical_shift, coordinate_ulp,
                             neighbour_gradient, rigid_resample_stack)

pytestmark = pytest.mark.gpu

GRIDS = ("catmull_rom", "bspline")


def _shift_table(t, values, offset=0):
    """(t, 2) integer shifts cycling through `values`, the two axes out of step."""
    v = list(values)
    return torch.tensor([[v[(offset + f) % len(v)], v[(offset + 3 * f + 1) % len(v)]] for f in range(t)],
                        dtype=torch.float32)


# ------------------------------------------------------------------ a. the pipeline's tables


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("ps", TABLE_SPACINGS)
def test_pipeline_tables_equal_the_generic_route(mc, dev, ps, grid):
    """engine.rigid_tables_from_shifts (rigid_tail + rigid_weights) against image_shifts_to_deformation_field +
    frame_lattices + rigid_tables: the field, shifts_px and the defined region of the scratch ([Wy | Wx | S] as
    mc_rigid_tables_from_shifts lays it out) bit for bit; shifts_px also against the canonical value computed on
    the CPU, and the shift route warp / warp_rigid_raw take without tables (engine.rigid_shifts_px)."""
    from torch_motion_correction_amd import engine

    for t in (1, 2, 3, 4, 6, 40):
        for h, w, values in ((64, 96, SMALL_SHIFTS), (130, 250, SMALL_SHIFTS), (512, 512, SMALL_SHIFTS + LARGE_SHIFTS)):
            sh = _shift_table(t, values, offset=t).to(dev)
            field_p, (sp_p, scr_p) = engine.rigid_tables_from_shifts(sh, (t, h, w), ps, grid)
            field_g = mc.image_shifts_to_deformation_field(sh, ps).contiguous()
            lat = engine.frame_lattices(field_g, t, grid)
            sp_g, scr_g = engine.rigid_tables(torch.empty((t, h, w), device=dev), lat, ps)
            n = t * 5 * (h + w) + 2 * t  # Wy, Wx (fp32), S (int32)
            case = (t, h, w)
            assert torch.equal(field_p, field_g), case
            assert torch.equal(sp_p, sp_g), (case, sp_p, sp_g)
            assert torch.equal(scr_p[:n].view(torch.int32), scr_g[:n].view(torch.int32)), case
            assert torch.equal(engine.rigid_shifts_px(lat, ps), sp_p), case
            # the canonical rule: the GPU lattice, divided on the CPU.  Even catmull_rom's L is not always
            # fp32(s * ps): the last frame's spline coordinate (1 - pos[t-2]) (t-1) is 1 only up to rounding
            want = lat[:, :, 0, 0].cpu().numpy() / np.float32(ps)
            assert np.array_equal(sp_p.cpu().numpy(), want), (case, sp_p.cpu().numpy(), want)
            if grid == "catmull_rom" and t > 1:  # the nodes before the last are exact: fp32(fp32(s * ps) / ps)
                assert np.array_equal(want[:-1], canonical_shift(sh[:-1].cpu().numpy(), ps)), case


# ------------------------------------------------------------------ b. frames against the float64 resampler


def _frame_bound(ref, mag, h, w):
    """Per-pixel bound of |kernel - float64 resampler|.  The kernels compute the sampling coordinate with the
    resampler's fp32 chain, so what differs is (1) fp32 arithmetic: each of the 16 products carries two fp32 cubic
    weights (a Horner chain of <= 8 roundings each, i.e. <= 8 ulp) and the separable 4 + 4-term sums add <= 8 more:
    32 ulp (2^-24 each) of sum |wy wx v|; and (2) for the general-field kernel, whose per-pixel shift is the bicubic
    upsample of the constant lattice, one coordinate ulp per axis moves the sample by at most ulp x the largest
    neighbour difference of its footprint (x 1.5: bicubic overshoot) -- assert_frames_close_large's rule."""
    return 32 * 2.0 ** -24 * mag + 2 * 1.5 * coordinate_ulp(h, w) * neighbour_gradient(ref)


@pytest.mark.parametrize("ps", FRAME_SPACINGS)
@pytest.mark.parametrize("shape", [(6, 128, 160), (4, 130, 250)])
def test_rigid_frames_match_the_float64_resampler(mc, dev, shape, ps):
    from torch_motion_correction_amd import api, engine

    t, h, w = shape
    g = torch.Generator().manual_seed(t * h + w)
    st = torch.randn(t, h, w, generator=g) * 2 + 5  # no pixel is zero by chance
    px = _shift_table(t, (-3, -5, -6, -10, 3, 5, 6, 9, -9, 13, -13, 15, -15, 7, -7, 0))
    field = mc.image_shifts_to_deformation_field(px, ps).contiguous()
    fd = field.to(dev)
    lat = engine.frame_lattices(fd, t, "catmull_rom")
    sh = lat[:, :, 0, 0].cpu().numpy() / np.float32(ps)  # the canonical rule, on the CPU
    # the general-field kernel's per-pixel shift is the bicubic upsample of the constant lattice over ps, a few
    # ulp off L / ps and varying along the frame (the reference's own knife edge): where the exact
    # coordinate p + s lies within a few ulp of the shift of the border, 0 or n - 1, its zero rule may go either
    # way.  Nowhere else.
    p_y, p_x = np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32)
    cy, cx = p_y[None, :] + sh[:, :1], p_x[None, :] + sh[:, 1:]
    eps = 8 * np.spacing(np.abs(sh))  # a few ulp of the shift: the upsample's rounding
    near = lambda c, n, e: (np.abs(c) <= e) | (np.abs(c - (n - 1)) <= e)  # noqa: E731
    on_border = near(cy, h, eps[:, :1])[:, :, None] | near(cx, w, eps[:, 1:])[:, None, :]
    for dtype in (torch.float32, torch.float16):
        src = st.to(dtype)
        sd = src.to(dev)
        ref, mag = rigid_resample_stack(src.float().numpy(), sh)
        bound = _frame_bound(ref, mag, h, w)
        sum_bound = bound.sum(0) + t * 2.0 ** -24 * np.abs(ref).sum(0)
        routes = {}
        routes["motion_correct_sum"] = mc.motion_correct_sum(sd, fd, ps, return_frames=True)[::-1]
        tables = engine.rigid_tables(sd, lat, ps)
        routes["warp(tables)"] = engine.warp(sd, None, ps, want_frames=True, want_sum=True, rigid=True,
                                             tables=tables)
        api.RIGID_FAST_PATH = False
        try:
            routes["general kernel"] = (mc.correct_motion(sd, fd, ps), mc.motion_correct_sum(sd, fd, ps))
        finally:
            api.RIGID_FAST_PATH = True
        for name, (frames, total) in routes.items():
            what = f"{name} {dtype} ps={ps}"
            _assert_frames(frames, ref, bound, what, on_border if name == "general kernel" else None)
            d = np.abs(total.cpu().double().numpy() - ref.sum(0))
            if name == "general kernel":
                # a pixel whose zero rule went the other way moves the sum by at most its two values
                d -= (on_border * (np.abs(ref) + np.abs(frames.cpu().double().numpy()))).sum(0)
            assert bool((d <= sum_bound).all()), (what, float((d - sum_bound).max()))


# ------------------------------------------------------------------ c. pipeline == per-call, exact


def _drift_movie(dy, dx, h, w, seed, pad=64, noise=0.3):
    """drift_stack's recipe (white-noise texture cropped at integer offsets + noise) with a given drift.  The noise
    is lower than drift_stack's: at ps = 0.83 the band-pass keeps a narrower share of the spectrum, and with noise
    1.0 the reference's own estimate misses some of these drifts by a pixel."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(h + 2 * pad, w + 2 * pad, generator=g)
    return torch.stack([base[pad - a: pad - a + h, pad - b: pad - b + w] + noise * torch.randn(h, w, generator=g)
                        for a, b in zip(dy, dx)])


# drift per movie; relative to the default reference frame (t // 2) it contains -3, -5 and -6 on both axes
_DRIFTS = {
    2: ([-3, 0], [-5, 0]),
    3: ([-5, 0, -6], [-6, 0, -3]),
    4: ([-3, -5, 0, -6], [-6, -3, 0, -5]),
    6: ([-3, -5, -6, 0, 4, 2], [-6, -3, -5, 0, 3, -2]),
}


@pytest.fixture(scope="module")
def pipeline_movies(dev):
    movies = []
    for i, (t, h, w) in enumerate([(2, 512, 512), (3, 512, 512), (6, 512, 512), (4, 256, 4096)]):
        dy, dx = _DRIFTS[t]
        movies.append((_drift_movie(dy, dx, h, w, seed=300 + i) * (1.0 + i) + 2.0 * i).to(dev))
    dy, dx = _DRIFTS[6]
    movies.append(_drift_movie(dy, dx, 512, 512, seed=399).half().to(dev))  # K1 and the warp read fp16
    return movies


@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("ps", PIPELINE_SPACINGS)
def test_pipeline_equals_per_call_routes(mc, dev, pipeline_movies, ps, grid, overlap):
    """MoviePipeline.run and motion_correct_movies return, movie by movie, exactly estimate_global_motion +
    motion_correct_sum(grid_type=grid): t = 2, 3, 6 at 512^2, a (4, 256, 4096) movie (wave K1 engine,
    warp_rigid_dma) and an fp16 movie; reference frame None, 0 and -1.  The recovered shifts equal the drift."""
    movies = pipeline_movies
    for ref in (None, 0, -1):
        runs = {"MoviePipeline.run": mc.MoviePipeline(dev, ps, reference_frame=ref, grid_type=grid,
                                                      return_frames=True, overlap=overlap).run(movies),
                "motion_correct_movies": mc.motion_correct_movies(movies, ps, reference_frame=ref, grid_type=grid,
                                                                  return_frames=True, overlap=overlap)}
        torch.cuda.synchronize()
        for m, r_a, r_b in zip(movies, runs["MoviePipeline.run"], runs["motion_correct_movies"]):
            t = m.shape[0]
            field = mc.estimate_global_motion(m, ps, reference_frame=ref)
            total, frames = mc.motion_correct_sum(m, field, ps, grid_type=grid, return_frames=True)
            dy, dx = _DRIFTS[t]
            r0 = t // 2 if ref is None else ref % t
            truth = torch.tensor([[a - dy[r0] for a in dy], [b - dx[r0] for b in dx]], dtype=torch.float32) * ps
            assert torch.equal(field[:, :, 0, 0].cpu(), truth), (tuple(m.shape), ref, field.flatten())
            for name, r in (("MoviePipeline.run", r_a), ("motion_correct_movies", r_b)):
                case = (name, tuple(m.shape), m.dtype, ref)
                assert torch.equal(r.field, field), case
                assert torch.equal(r.frames, frames), case
                assert torch.equal(r.total, total), case


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("ps", PIPELINE_SPACINGS)
def test_single_frame_movie_takes_the_same_route_everywhere(mc, dev, ps, grid):
    """t = 1: the time spline has one sample (spline.axis_taps clamps the index).  The pipeline and the per-call
    route give the same bits, or refuse it with the same error."""
    m = _drift_movie([0], [0], 512, 512, seed=77).to(dev)

    def per_call():
        field = mc.estimate_global_motion(m, ps)
        return (field, *mc.motion_correct_sum(m, field, ps, grid_type=grid, return_frames=True))

    def pipeline():
        r = mc.MoviePipeline(dev, ps, grid_type=grid, return_frames=True).run([m])[0]
        return r.field, r.total, r.frames

    out = []
    for fn in (per_call, pipeline):
        try:
            out.append(fn())
        except Exception as e:  # noqa: BLE001 -- both routes must refuse alike
            out.append((type(e), str(e)))
    torch.cuda.synchronize()
    a, b = out
    if isinstance(a[0], type) or isinstance(b[0], type):
        assert a == b
        return
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert float(a[0].abs().max()) == 0.0


# ------------------------------------------------------------------ d. raw movies


@pytest.fixture(scope="module")
def raw_movies(dev):
    dy, dx = _DRIFTS[4]
    out = {}
    for dtype in (torch.uint8, torch.int16):
        out[dtype] = [drifting_raw_movie(dy, dx, 256, 4096, dtype, seed=500 + i).to(dev) for i in range(3)]
    gain = (1.0 + 0.1 * torch.randn(256, 4096, generator=torch.Generator().manual_seed(9))).clamp(0.5, 1.5)
    return out, gain.to(dev)


@pytest.mark.parametrize("with_gain", [True, False])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("ps", RAW_SPACINGS)
def test_raw_pipeline_equals_one_call_per_movie(mc, dev, raw_movies, ps, grid, dtype, with_gain):
    movies, gain = raw_movies
    movies = movies[dtype]
    gd = gain if with_gain else None
    res = mc.RawMoviePipeline(gd, dev, ps, grid_type=grid, return_frames=True, overlap=True).run(movies)
    torch.cuda.synchronize()
    dy, dx = _DRIFTS[4]
    truth = torch.tensor([[a - dy[2] for a in dy], [b - dx[2] for b in dx]], dtype=torch.float32) * ps
    for i, (m, r) in enumerate(zip(movies, res)):
        f, s, fr = mc.motion_correct_raw(m, gd, ps, grid_type=grid, return_frames=True)
        assert torch.equal(r.field, f), i
        assert torch.equal(f[:, :, 0, 0].cpu(), truth), (i, f.flatten())
        assert torch.equal(r.frames, fr), i
        assert torch.equal(r.total, s), i


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
def test_raw_route_equals_conditioning_then_the_fp32_route(mc, dev, raw_movies, dtype):
    """At ps = 0.83 motion_correct_raw (the fused raw warp, and with a dose the rigid shift route of
    warp_dose_weighted_sum_raw) against condition_movie -> estimate_global_motion -> motion_correct_sum, with the
    tolerances of the ps = 1 tests (the roundings of raw * gain - mu differ in the last bit): field exact, images to
    1e-5 of their range (the dose-weighted sums 2e-5).  The zero pattern of the frames is the canonical one, and the
    streamed dose-weighted sum equals the dose filter of the pipeline's frames."""
    from torch_motion_correction_amd import engine

    ps = 0.83
    movies, gd = raw_movies
    m = movies[dtype][0]
    t, h, w = m.shape
    f, s, fr = mc.motion_correct_raw(m, gd, ps, return_frames=True)
    img = mc.condition_movie(m, gd)
    fa = mc.estimate_global_motion(img, ps)
    sa, fra = mc.motion_correct_sum(img, fa, ps, return_frames=True)
    assert torch.equal(f, fa)
    assert rel_err(fr, fra) <= 1e-5 and rel_err(s, sa) <= 1e-5
    sh = engine.frame_lattices(fa, t, "catmull_rom")[:, :, 0, 0].cpu().numpy() / np.float32(ps)
    p_y, p_x = np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32)
    for i in range(t):
        cy, cx = p_y + sh[i, 0], p_x + sh[i, 1]
        zero = ~(((cy >= 0) & (cy <= h - 1))[:, None] & ((cx >= 0) & (cx <= w - 1))[None, :])
        for frames in (fr, fra):
            assert np.array_equal(frames[i].cpu().numpy() == 0, zero), i
    dose = dict(dose_per_frame=1.3, pre_exposure=0.5)
    f_d, dw = mc.motion_correct_raw(m, gd, ps, **dose)
    dw_c = mc.motion_correct_sum(img, fa, ps, **dose)
    assert torch.equal(f_d, f)
    assert rel_err(dw, dw_c) <= 2e-5, rel_err(dw, dw_c)
    piped = mc.RawMoviePipeline(gd, dev, ps, return_frames=True).run([m])[0]
    torch.cuda.synchronize()
    assert rel_err(dw, mc.dose_weighted_sum(piped.frames, ps, **dose)) <= 2e-5
