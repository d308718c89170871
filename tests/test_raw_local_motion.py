"""The fused raw local-motion route (motion_correct_raw_patches, engine.patch_field_raw, engine.warp_field_raw):
results equal condition_movie followed by the patch estimator and the deformation-field warp, without a
conditioned fp32 movie."""

import numpy as np
import pytest
import torch

import oracle
from oracle import thirdparty_semantics as tp
from torch_motion_correction_amd import engine
from torch_motion_correction_amd._lib import McorrUnsupported

pytestmark = pytest.mark.gpu

REL = 1e-4


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def local_motion_stack(mc, dev, t, h, w, gh, gw, amp, seed, noise=0.5):
    """A texture seen through a smooth, small (|shift| <= amp px) local deformation that varies in time, built on
    the GPU with the product's own warp (the generator of the patch-estimator parity tests)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    base = torch.randn(h, w, generator=g, device=dev)
    base = (base + torch.roll(base, 1, 0) + torch.roll(base, 1, 1) + torch.roll(base, (1, 1), (0, 1))) / 2
    tt = torch.linspace(-1, 1, t)[:, None, None]
    yy = torch.linspace(-1, 1, gh)[None, :, None]
    xx = torch.linspace(-1, 1, gw)[None, None, :]
    true = torch.stack([amp * tt * torch.sin(2.0 * yy + 1.0 * xx), amp * tt * torch.cos(1.5 * xx - yy)])
    frames = torch.empty((t, h, w), dtype=torch.float32, device=dev)
    for f in range(t):
        one = mc.correct_motion(base[None], -true[:, f:f + 1].to(dev), 1.0, grid_type="bspline")[0]
        frames[f] = one + noise * torch.randn(h, w, generator=g, device=dev)
    return frames, true


def raw_movie(frames, dtype, seed):
    """Detector counts of the frames: u8 around 100, or i16 with an offset, divided by a gain of 1 +- 0.1."""
    h, w = frames.shape[-2:]
    g = torch.Generator(device=frames.device).manual_seed(seed)
    gain = (1.0 + 0.1 * (2 * torch.rand(h, w, generator=g, device=frames.device) - 1))
    if dtype == torch.uint8:
        raw = ((frames * 20 + 100) / gain).round().clamp(0, 255).to(torch.uint8)
    else:
        raw = ((frames * 160 - 300) / gain).round().clamp(-32768, 32767).to(torch.int16)
    return raw, gain


def rel_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


@pytest.fixture(scope="module")
def c3_frames(mc, dev):
    frames, _ = local_motion_stack(mc, dev, 6, 4092, 5760, 6, 10, 2.0, seed=3)
    return frames


PATCH_KW = dict(b_factor=500.0, frequency_range=(300, 10), patch_sidelength=1024, sub_pixel_refinement=True,
                temporal_smoothing=True, smoothing_window_size=5, outlier_rejection=True, outlier_threshold=3.0)


@pytest.mark.parametrize("dtype,strategy,ref", [(torch.uint8, "mean_except_current", 3),
                                                (torch.int16, "mean_except_current", 3),
                                                (torch.uint8, "middle_frame", 0),
                                                (torch.int16, "middle_frame", -1)])
def test_patch_estimator_from_raw_bytes(mc, dev, c3_frames, dtype, strategy, ref):
    """BASELINE C3 size (6 x 4092 x 5760, 6 x 10 patches of 1024 px): patch_field_raw on the raw bytes against
    patch_field on condition_movie's fp32 movie."""
    raw, gain = raw_movie(c3_frames, dtype, seed=11)
    img = engine.condition_movie(raw, gain)
    stats = engine.central_box_stats(img)
    want, wpos = engine.patch_field(img, stats, 1.0, ref, strategy, field0=None, **PATCH_KW)
    del img
    rm = engine.RawMovie(raw, gain)
    got, gpos = engine.patch_field_raw(rm, 1.0, ref, strategy, **PATCH_KW)
    assert tuple(got.shape) == (2, 6, 6, 10) and torch.equal(gpos, wpos)
    assert float((got - want).abs().max()) <= 1e-4
    assert float(want.abs().max()) > 0.3  # a real field, not zeros


def _field(t, gh, gw, amp, seed):
    g = torch.Generator().manual_seed(seed)
    return amp * (2 * torch.rand(2, t, gh, gw, generator=g) - 1)


@pytest.mark.parametrize("case", ["u8", "i16", "large_field", "no_gain", "not_mean_zero"])
@pytest.mark.parametrize("grid_type", ["catmull_rom", "bspline"])
def test_field_warp_from_raw_bytes(mc, dev, case, grid_type):
    """warp_field_raw against motion_correct_sum of the conditioned movie with the same field: frames and sum.  Every
    frame's windows cross the frame border (zero-outside rule); the large field sends tiles to the slow kernel."""
    t, h, w, ps = 5, 1100, 1536, 1.3
    frames, _ = local_motion_stack(mc, dev, t, h, w, 3, 4, 1.5, seed=7)
    raw, gain = raw_movie(frames, torch.int16 if case == "i16" else torch.uint8, seed=5)
    if case == "no_gain":
        gain = None
    mean_zero = case != "not_mean_zero"
    field = _field(t, 4, 5, 40.0 if case == "large_field" else 3.0, seed=2).to(dev)
    img = mc.condition_movie(raw, gain, mean_zero=mean_zero)
    want_sum, want_frames = mc.motion_correct_sum(img, field, ps, grid_type=grid_type, return_frames=True)
    rm = engine.RawMovie(raw, gain, mean_zero=mean_zero)
    lat = engine.frame_lattices(field, t, grid_type)
    got_frames, got_sum = engine.warp_field_raw(rm, lat, ps, want_frames=True, want_sum=True)
    assert rel_err(got_frames, want_frames) <= 1e-5
    assert rel_err(got_sum, want_sum) <= 1e-5
    # the border: some outputs sample outside the frame and are exactly zero in both
    zero = want_frames == 0
    assert bool(zero.any()) and bool((got_frames[zero] == 0).all())
    if case == "large_field":
        # irregular tiles really took the slow kernel: its output is there, not left at zero
        assert float(got_frames.abs().mean()) > 0.5 * float(want_frames.abs().mean())
    _, only_sum = engine.warp_field_raw(rm, lat, ps, want_frames=False, want_sum=True)
    assert torch.equal(only_sum, got_sum)


def knife_edge_mask(stack, field, pixel_spacing, grid_type, eps=1e-3):
    """(t,h,w) bool: oracle sampling coordinate within eps of the frame border."""
    t, h, w = stack.shape
    _, _, gh, gw = field.shape
    grid = tp.coordinate_grid((h, w))
    out = torch.zeros(t, h, w, dtype=torch.bool)
    for i, ft in enumerate(torch.linspace(0, 1, steps=t)):
        lat = oracle.evaluate_deformation_field_at_t(field, ft, (10 * gh, 10 * gw), grid_type)
        c = grid + oracle.get_pixel_shifts(stack[i], pixel_spacing, lat, grid)
        near = lambda v, n: (v.abs() < eps) | ((v - (n - 1)).abs() < eps)  # noqa: E731
        out[i] = near(c[..., 0], h) | near(c[..., 1], w)
    return out


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
def test_end_to_end_against_the_oracle(mc, dev, dtype):
    """motion_correct_raw_patches at a reduced frame size with 1024-px patches against the oracle run on the
    example's numpy conditioning (float64 raw * gain - frame mean)."""
    t, h, w = 5, 1536, 2048
    frames, _ = local_motion_stack(mc, dev, t, h, w, 3, 4, 2.0, seed=9)
    raw, gain = raw_movie(frames, dtype, seed=4)
    field, pos, total = mc.motion_correct_raw_patches(raw, gain, 1.0, grid_type="bspline")
    x = raw.cpu().numpy().astype(np.float64) * gain.cpu().numpy().astype(np.float64)
    cond = torch.from_numpy((x - x.mean(axis=(1, 2), keepdims=True)).astype(np.float32))
    ofield, opos = oracle.estimate_motion_cross_correlation_patches(cond, 1.0, patch_sidelength=1024)
    assert torch.equal(pos.cpu(), opos)
    assert float((field.cpu() - ofield).abs().max()) <= REL
    oframes = oracle.correct_motion(cond, ofield, 1.0, grid_type="bspline")
    knife = knife_edge_mask(cond, ofield, 1.0, "bspline")
    assert float(knife.float().mean()) <= 0.02
    osum = oframes.sum(0)
    d = (total.cpu() - osum).abs()
    d[knife.any(0)] = 0
    assert float((d > 2 * REL * float(osum.abs().max())).float().mean()) <= 2e-2
    assert float(d.max()) <= 20 * REL * float(osum.abs().max())


def test_no_fp32_movie_is_allocated(mc, dev, c3_frames):
    """6 x 4092 x 5760 u8: the fused route's peak stays below the conditioned route's by 0.9 of an fp32 movie."""
    raw, gain = raw_movie(c3_frames, torch.uint8, seed=11)
    t, h, w = raw.shape
    torch.cuda.synchronize()

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        used = torch.cuda.max_memory_allocated() - base
        del out
        return used

    def conditioned():
        img = mc.condition_movie(raw, gain)
        field, pos = mc.estimate_motion_cross_correlation_patches(img, 1.0, patch_sidelength=1024)
        return field, pos, mc.motion_correct_sum(img, field, 1.0)

    fused = lambda: mc.motion_correct_raw_patches(raw, gain, 1.0)  # noqa: E731
    fused()  # plans and tables built once outside the measured calls
    conditioned()
    p_cond, p_fused = peak(conditioned), peak(fused)
    assert p_fused <= p_cond - 0.9 * 4 * t * h * w, (p_fused, p_cond)


@pytest.fixture(scope="module")
def small_case(mc, dev):
    frames, _ = local_motion_stack(mc, dev, 5, 1100, 1536, 3, 4, 1.5, seed=13)
    return raw_movie(frames, torch.uint8, seed=6)


def _conditioned_route(mc, movie, gain, hot=None, **kw):
    img = mc.condition_movie(movie, gain, hot_pixel_threshold=hot)
    est = {k: v for k, v in kw.items() if k != "grid_type"}
    field, pos = mc.estimate_motion_cross_correlation_patches(img, 1.0, **est)
    total = mc.motion_correct_sum(img, field, 1.0, grid_type=kw.get("grid_type", "catmull_rom"))
    return field, pos, total


@pytest.mark.parametrize("case", ["patch512", "hot_pixels", "prior_field", "fp16"])
def test_fallbacks_are_exactly_the_conditioned_route(mc, dev, small_case, case):
    raw, gain = small_case
    kw = dict(patch_sidelength=512) if case == "patch512" else {}
    hot = 10.0 if case == "hot_pixels" else None
    if case == "prior_field":
        kw["deformation_field"] = _field(5, 2, 2, 2.0, seed=8).to(dev)
    movie = raw.to(torch.float16) if case == "fp16" else raw
    got = mc.motion_correct_raw_patches(movie, gain, 1.0, hot_pixel_threshold=hot, **kw)
    want = _conditioned_route(mc, movie, gain, hot=hot, **kw)
    assert len(got) == 3
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_fused_route_is_taken(mc, dev, small_case, monkeypatch):
    raw, gain = small_case
    want = _conditioned_route(mc, raw, gain)

    def refuse(*a, **k):
        raise AssertionError("the fused route conditioned the movie")

    monkeypatch.setattr(engine, "condition_movie", refuse)
    field, pos, total, frames = mc.motion_correct_raw_patches(raw, gain, 1.0, return_frames=True)
    assert torch.equal(pos, want[1]) and float((field - want[0]).abs().max()) <= 1e-4
    assert rel_err(total, want[2]) <= 1e-4 and rel_err(frames.sum(0), want[2]) <= 1e-4


def test_unsupported_shapes_raise(mc, dev, small_case):
    raw, gain = small_case
    rm = engine.RawMovie(raw, gain)
    with pytest.raises(McorrUnsupported):
        engine.patch_field_raw(rm, 1.0, 2, "mean_except_current", **dict(PATCH_KW, patch_sidelength=512))
    odd = engine.RawMovie(raw[:, :, :1000].contiguous(), gain[:, :1000])  # rows of 1000 u8 samples
    lat = engine.frame_lattices(_field(5, 3, 4, 2.0, seed=1).to(dev), 5, "catmull_rom")
    with pytest.raises(McorrUnsupported):
        engine.warp_field_raw(odd, lat, 1.0, want_frames=False, want_sum=True)
    hot = engine.RawMovie(raw, gain, hot_pixel_threshold=10.0)
    with pytest.raises(McorrUnsupported):
        engine.warp_field_raw(hot, lat, 1.0, want_frames=False, want_sum=True)
