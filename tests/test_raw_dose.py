"""Dose-weighted sums straight from raw u8 / i16 movies (motion_correct_sum_raw, motion_correct_raw(dose_per_frame=...),
engine.warp_dose_weighted_sum_raw): the exposure-filtered sum equals condition_movie followed by
motion_correct_sum(dose_per_frame=...), the plain sum comes from the same warp launches (accumulated across the
chunks of frames), and no conditioned fp32 movie is allocated.

The chunking test pins the accumulating kernels bit for bit against ((s_0 + s_1) + s_2) + s_3 of per-chunk sums.
Its field is small enough that no tile-frame goes to warp_field_slow: when that kernel runs, a chunk adds
(old + fast) + slow, which is not old + (fast + slow) in fp32."""

import numpy as np
import pytest
import torch

import oracle
from kernel_harness import mc, rel_err, switches  # noqa: F401
from oracle import thirdparty_semantics as tp
from torch_motion_correction_amd import _lib, engine

pytestmark = pytest.mark.gpu

REL = 2e-5
HOT = 10.0


def raw_movie(dev, t, h, w, dtype, seed, hot=False):
    """Detector counts of a smooth texture at a few integer offsets + noise (u8 around 100, i16 with an offset), a
    gain reference of 1 +- 0.1; with `hot`, hot pixels at the corners, on the edges, as adjacent pairs and at random
    positions per frame (gain 1 there), as tests/test_raw_hot_pixels.py plants them."""
    g = torch.Generator(device=dev).manual_seed(seed)
    base = torch.rand(h + 16, w + 16, generator=g, device=dev)
    base = (base + torch.roll(base, 1, 0) + torch.roll(base, 1, 1) + torch.roll(base, (1, 1), (0, 1))) / 4
    gain = 1.0 + 0.1 * (2 * torch.rand(h, w, generator=g, device=dev) - 1)
    raw = torch.empty((t, h, w), dtype=dtype, device=dev)
    for f in range(t):
        oy, ox = 4 + (f * 3) % 7 - 3, 4 + (f * 5) % 9 - 4
        v = 60 * base[4 + oy:4 + oy + h, 4 + ox:4 + ox + w] + 5 * torch.randn(h, w, generator=g, device=dev)
        if dtype == torch.uint8:
            raw[f] = ((v + 70) / gain).round().clamp(0, 255).to(dtype)
        else:
            raw[f] = ((8 * v - 300) / gain).round().clamp(-32768, 32767).to(dtype)
    if hot:
        hi = 255 if dtype == torch.uint8 else 30000
        for y, x in [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 3), (h - 1, w // 2 + 5), (h // 3, 0),
                     (h // 2 + 3, w - 1), (h // 2, w // 2), (h // 2, w // 2 + 1), (1, 1), (h - 2, w - 2)]:
            raw[:, y, x] = hi
            gain[y, x] = 1.0
        for f in range(t):
            ys = torch.randint(0, h, (6,), generator=g, device=dev)
            xs = torch.randint(0, w, (6,), generator=g, device=dev)
            raw[f, ys, xs] = hi
            gain[ys, xs] = 1.0
    return raw, gain


def make_field(dev, t, gh, gw, amp, seed):
    g = torch.Generator().manual_seed(seed)
    return (amp * (2 * torch.rand(2, t, gh, gw, generator=g) - 1)).to(dev)


def conditioned(mc, movie, gain, field, ps, mean_zero=True, hot=None, grid_type="catmull_rom", **dose):
    """The conditioned route: condition_movie, then motion_correct_sum with and without the dose."""
    img = mc.condition_movie(movie, gain, mean_zero=mean_zero, hot_pixel_threshold=hot)
    dw = mc.motion_correct_sum(img, field, ps, grid_type=grid_type, **dose)
    plain = mc.motion_correct_sum(img, field, ps, grid_type=grid_type)
    return dw, plain


def refuse_conditioning(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the fused route conditioned the movie")

    monkeypatch.setattr(engine, "condition_movie", refuse)


# (dtype, field grid, grid_type, gain, mean_zero, hot, ps, pre_exposure, voltage)
CASES = {
    "u8_rigid": (torch.uint8, (1, 1), "catmull_rom", True, True, None, 1.0, 0.0, 300.0),
    "i16_rigid_bspline": (torch.int16, (1, 1), "bspline", True, True, None, 1.0, 0.0, 300.0),
    "u8_local": (torch.uint8, (3, 4), "catmull_rom", True, True, None, 1.0, 0.0, 300.0),
    "i16_local_bspline": (torch.int16, (3, 4), "bspline", True, True, None, 1.0, 0.0, 300.0),
    "u8_local_1x4": (torch.uint8, (1, 4), "bspline", True, True, None, 1.0, 0.0, 300.0),
    "no_gain": (torch.uint8, (1, 1), "catmull_rom", False, True, None, 1.0, 0.0, 300.0),
    "not_mean_zero": (torch.int16, (1, 4), "catmull_rom", True, False, None, 1.0, 0.0, 300.0),
    "hot_rigid": (torch.uint8, (1, 1), "catmull_rom", True, True, HOT, 1.0, 0.0, 300.0),
    "ps_pre_voltage_local": (torch.uint8, (1, 4), "catmull_rom", True, True, None, 1.3, 2.0, 200.0),
    "ps_pre_voltage_rigid": (torch.int16, (1, 1), "bspline", True, True, None, 0.8, 1.0, 200.0),
}


def _fused_kernel_exists(h, grid):
    """mc_warp_frames_raw takes the reference's sparse lattice only: 32 pixel rows span <= 1.5 lattice cells."""
    return grid == (1, 1) or 32 * (10 * grid[0] - 1) * 2 <= 3 * (h - 1)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("shape", [(7, 256, 512), (5, 512, 1024), (3, 4092, 5760)])
def test_fused_equals_the_conditioned_route(mc, dev, shape, case, monkeypatch):
    dtype, grid, grid_type, with_gain, mean_zero, hot, ps, pre, volt = CASES[case]
    t, h, w = shape
    raw, gain = raw_movie(dev, t, h, w, dtype, seed=t + h, hot=hot is not None)
    gain = gain if with_gain else None
    field = make_field(dev, t, *grid, 3.0 * ps, seed=len(case))
    dose = dict(dose_per_frame=1.1, pre_exposure=pre, voltage=volt)
    want_dw, want_plain = conditioned(mc, raw, gain, field, ps, mean_zero, hot, grid_type, **dose)
    if _fused_kernel_exists(h, grid):  # the fused route really is taken
        refuse_conditioning(monkeypatch)
    dw, plain = mc.motion_correct_sum_raw(raw, gain, field, ps, grid_type=grid_type, mean_zero=mean_zero,
                                          hot_pixel_threshold=hot, return_plain_sum=True, **dose)
    assert rel_err(dw, want_dw) <= REL, rel_err(dw, want_dw)
    assert rel_err(plain, want_plain) <= REL, rel_err(plain, want_plain)
    assert float(want_dw.abs().max()) > 0


@pytest.mark.parametrize("rigid", [True, False])
def test_chunks_accumulate_the_plain_sum_in_order(mc, dev, switches, rigid):
    """Two frames per chunk, 7 frames: chunks [0,2) [2,4) [4,6) [6,7)."""
    t, h, w, ps = 7, 1024, 1024, 1.0
    raw, gain = raw_movie(dev, t, h, w, torch.uint8, seed=5)
    # +-0.6 px: half the node range over any tile's support is <= 0.6 px, far inside warp_field_plan's regular
    # windows (3.8 r + 1.05 <= 6), so no tile-frame takes warp_field_slow
    field = make_field(dev, t, 1 if rigid else 3, 1 if rigid else 4, 0.6, seed=9)
    grid_type = "catmull_rom"
    dose = dict(dose_per_frame=0.9, pre_exposure=0.5, voltage=200.0)
    whole_plain = mc.motion_correct_sum_raw(raw, gain, field, ps)
    pitch = _lib.load().mc_full_spectrum_pitch(w)
    ws, engine.WORKSPACE_BYTES = engine.WORKSPACE_BYTES, 2 * h * pitch * 8
    dw, plain = mc.motion_correct_sum_raw(raw, gain, field, ps, return_plain_sum=True, **dose)
    want_dw, _ = conditioned(mc, raw, gain, field, ps, **dose)
    engine.WORKSPACE_BYTES = ws
    assert rel_err(dw, want_dw) <= REL
    rm = engine.RawMovie(raw, gain)
    lat = engine.frame_lattices(field, t, grid_type)
    warp = engine.warp_rigid_raw if rigid else engine.warp_field_raw
    sums = [warp(rm.window(a, n), lat[a:a + n], ps, want_frames=True, want_sum=True)[1]
            for a, n in ((0, 2), (2, 2), (4, 2), (6, 1))]
    assert torch.equal(plain, ((sums[0] + sums[1]) + sums[2]) + sums[3])
    assert not torch.equal(sums[0], sums[1])
    assert rel_err(plain, whole_plain) <= 1e-6


def test_rigid_plain_sum_equals_motion_correct_raw(mc, dev):
    raw, gain = raw_movie(dev, 6, 512, 4096, torch.uint8, seed=3)
    field, total = mc.motion_correct_raw(raw, gain, 1.0)
    assert float(field.abs().max()) >= 1  # a real drift
    assert torch.equal(mc.motion_correct_sum_raw(raw, gain, field, 1.0), total)


def test_local_plain_sum_equals_motion_correct_raw_patches(mc, dev):
    raw, gain = raw_movie(dev, 5, 1536, 2048, torch.int16, seed=4)
    field, _, total = mc.motion_correct_raw_patches(raw, gain, 1.0, grid_type="bspline")
    assert tuple(field.shape[-2:]) != (1, 1)
    assert torch.equal(mc.motion_correct_sum_raw(raw, gain, field, 1.0, grid_type="bspline"), total)


def test_motion_correct_raw_with_a_dose(mc, dev):
    t, ps = 6, 1.2
    raw, gain = raw_movie(dev, t, 512, 4096, torch.uint8, seed=8, hot=True)
    dose = dict(dose_per_frame=1.5, pre_exposure=0.5, voltage=200.0)
    field0, total0, frames0 = mc.motion_correct_raw(raw, gain, ps, return_frames=True, hot_pixel_threshold=HOT)
    # without a dose: the engine chain of the fused route, output for output
    rm = engine.RawMovie(raw, gain, hot_pixel_threshold=HOT)
    shifts = engine.global_shifts_raw(rm, t // 2, ps, 500.0, (300, 10))
    field_e = mc.image_shifts_to_deformation_field(shifts, ps)
    frames_e, total_e = engine.warp_rigid_raw(rm, engine.frame_lattices(field_e.contiguous(), t, "catmull_rom"), ps,
                                              want_frames=True, want_sum=True)
    assert torch.equal(field0, field_e) and torch.equal(total0, total_e) and torch.equal(frames0, frames_e)
    # with a dose: the same field, the dose-weighted sum of motion_correct_sum_raw
    field1, dw = mc.motion_correct_raw(raw, gain, ps, hot_pixel_threshold=HOT, **dose)
    assert torch.equal(field1, field0)
    assert torch.equal(dw, mc.motion_correct_sum_raw(raw, gain, field1, ps, hot_pixel_threshold=HOT, **dose))
    assert not torch.equal(dw, total0)
    field2, dw2, frames2 = mc.motion_correct_raw(raw, gain, ps, return_frames=True, hot_pixel_threshold=HOT, **dose)
    assert torch.equal(field2, field0) and torch.equal(frames2, frames0)
    assert torch.equal(dw2, mc.dose_weighted_sum(frames0, ps, **dose))
    assert rel_err(dw2, dw) <= REL


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


@pytest.mark.parametrize("shape,grid,grid_type", [((5, 512, 1024), (2, 3), "bspline"),
                                                  ((6, 256, 512), (1, 1), "catmull_rom")])
def test_against_the_oracle(mc, dev, shape, grid, grid_type, monkeypatch):
    """The example's numpy conditioning (float64 raw * gain - frame mean), then the oracle's correct_motion and
    dose_weighted_sum.  Pixels sampled within 1e-3 of the frame border are a discontinuity of the oracle's
    zero-outside rule: there the oracle's frames get ours before its dose weighting (and are left out of the frame
    comparison)."""
    t, h, w = shape
    ps, dose = 1.1, dict(dose_per_frame=1.3, pre_exposure=0.4, voltage=300.0)
    raw, gain = raw_movie(dev, t, h, w, torch.uint8, seed=12)
    field = make_field(dev, t, *grid, 3.0, seed=2)
    refuse_conditioning(monkeypatch)
    streamed, plain = mc.motion_correct_sum_raw(raw, gain, field, ps, grid_type=grid_type, return_plain_sum=True,
                                                **dose)
    _, frames = mc.motion_correct_sum_raw(raw, gain, field, ps, grid_type=grid_type, return_frames=True, **dose)
    x = raw.cpu().numpy().astype(np.float64) * gain.cpu().numpy().astype(np.float64)
    cond = torch.from_numpy((x - x.mean(axis=(1, 2), keepdims=True)).astype(np.float32))
    ofield = field.cpu()
    oframes = oracle.correct_motion(cond, ofield, ps, grid_type=grid_type)
    knife = knife_edge_mask(cond, ofield, ps, grid_type)
    assert float(knife.float().mean()) <= 0.02
    ours = frames.cpu()
    d = (ours - oframes).abs()
    d[knife] = 0
    assert float(d.max()) <= 1e-4 * float(oframes.abs().max())
    hybrid = torch.where(knife, ours, oframes)
    ref = oracle.dose_weighted_sum(hybrid, ps, **dose)
    assert float((streamed.cpu() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
    osum = hybrid.sum(0)
    assert float((plain.cpu() - osum).abs().max()) <= 1e-4 * float(osum.abs().max())


def test_no_fp32_movie_is_allocated(mc, dev):
    """12 x 8184 x 11520 u8 (BASELINE C5 frames), a 3 x 4 field: the fused route's peak stays below the conditioned
    route's by 0.9 of an fp32 movie."""
    t, h, w = 12, 8184, 11520
    raw, gain = raw_movie(dev, t, h, w, torch.uint8, seed=1)
    field = make_field(dev, t, 3, 4, 3.0, seed=3)
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

    fused = lambda: mc.motion_correct_sum_raw(raw, gain, field, 1.0, dose_per_frame=1.0)  # noqa: E731
    cond = lambda: mc.motion_correct_sum(mc.condition_movie(raw, gain), field, 1.0, dose_per_frame=1.0)  # noqa: E731
    fused()  # plans and tables built once outside the measured calls
    cond()
    p_cond, p_fused = peak(cond), peak(fused)
    assert p_fused <= p_cond - 0.9 * 4 * t * h * w, (p_fused, p_cond)


@pytest.mark.parametrize("grid", [(1, 1), (3, 4)])
def test_fused_route_is_taken(mc, dev, grid, monkeypatch):
    t, h, w = 4, 1024, 2048
    raw, gain = raw_movie(dev, t, h, w, torch.uint8, seed=6)
    field = make_field(dev, t, *grid, 2.0, seed=4)
    want_dw, want_plain = conditioned(mc, raw, gain, field, 1.0, dose_per_frame=1.0)
    refuse_conditioning(monkeypatch)
    dw, plain = mc.motion_correct_sum_raw(raw, gain, field, 1.0, dose_per_frame=1.0, return_plain_sum=True)
    dw_f, plain_f, frames = mc.motion_correct_sum_raw(raw, gain, field, 1.0, dose_per_frame=1.0, return_plain_sum=True,
                                                      return_frames=True)
    only = mc.motion_correct_sum_raw(raw, gain, field, 1.0)
    assert rel_err(dw, want_dw) <= REL and rel_err(dw_f, want_dw) <= REL
    assert rel_err(plain, want_plain) <= REL and rel_err(plain_f, want_plain) <= REL
    assert rel_err(only, want_plain) <= REL and tuple(frames.shape) == (t, h, w)


@pytest.mark.parametrize("case", ["not_row_major", "fp16", "fp32", "local_hot", "polyphase"])
def test_fallbacks_are_exactly_the_conditioned_route(mc, dev, case, monkeypatch):
    shape = (5, 1100, 1536) if case == "not_row_major" else (5, 512, 1024)
    raw, gain = raw_movie(dev, *shape, torch.uint8, seed=7, hot=case == "local_hot")
    movie = {"fp16": raw.to(torch.float16), "fp32": raw.to(torch.float32)}.get(case, raw)
    field = make_field(dev, shape[0], 2, 3, 2.0, seed=5)
    hot = HOT if case == "local_hot" else None
    if case == "polyphase":
        monkeypatch.setattr(engine, "POLYPHASE_FOURIER_SHIFT", True)
    dose = dict(dose_per_frame=1.2, pre_exposure=0.3, voltage=300.0)
    got = mc.motion_correct_sum_raw(movie, gain, field, 1.0, hot_pixel_threshold=hot, return_plain_sum=True, **dose)
    want = conditioned(mc, movie, gain, field, 1.0, hot=hot, **dose)
    assert len(got) == 2
    for a, b in zip(got, want):
        assert torch.equal(a, b)
