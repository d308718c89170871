"""Fused Fourier-shift sums straight from raw u8 / i16 movies (motion_correct_sum_fast_raw, motion_correct_raw_fast,
engine.fast_shift_sums on a RawMovie): the row transform reads the raw bytes, hot pixels enter the spectra as sparse
corrections, and no conditioned or shifted fp32 movie is allocated.  Without hot pixels the launches and samples are
those of motion_correct_sum_fast on condition_movie's output, so the sums are equal bit for bit."""

import pytest
import torch

from torch_motion_correction_amd import engine

pytestmark = pytest.mark.gpu

HOT = 10.0


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def range_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.max() - b.min()), 1e-30))


def raw_movie(dev, t, h, w, dtype, seed, hot=False):
    """Detector counts of a smooth texture at a few integer offsets + noise, a gain reference of 1 +- 0.1; with `hot`,
    hot pixels at the corners, on the edges, as adjacent pairs and at random positions per frame (gain 1 there), as
    tests/test_raw_dose.py plants them."""
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


def rigid_field(dev, t, amp, seed):
    g = torch.Generator().manual_seed(seed)
    return (amp * (2 * torch.rand(2, t, 1, 1, generator=g) - 1)).to(dev)


def refuse_conditioning(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the fused route conditioned the movie")

    monkeypatch.setattr(engine, "condition_movie", refuse)


# (dtype, gain, mean_zero, ps, dose, pre, kv)
CASES = {
    "u8": (torch.uint8, True, True, 1.0, 1.2, 0.0, 300.0),
    "i16": (torch.int16, True, True, 0.8, 0.9, 1.0, 200.0),
    "no_gain": (torch.uint8, False, True, 1.3, 1.0, 0.5, 300.0),
    "not_mean_zero": (torch.int16, True, False, 1.0, 1.5, 0.0, 100.0),
}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("shape", [(5, 512, 1024), (3, 4096, 256), (3, 4092, 5760)])
def test_without_hot_pixels_equals_the_conditioned_route(mc, dev, shape, case):
    dtype, with_gain, mean_zero, ps, dose, pre, kv = CASES[case]
    raw, gain = raw_movie(dev, *shape, dtype, seed=sum(shape))
    gain = gain if with_gain else None
    field = rigid_field(dev, shape[0], 5.0 * ps, seed=len(case))
    img = mc.condition_movie(raw, gain, mean_zero=mean_zero)
    want_plain = mc.motion_correct_sum_fast(img, field, ps)
    want = mc.motion_correct_sum_fast(img, field, ps, dose_per_frame=dose, pre_exposure=pre, voltage=kv,
                                      return_plain_sum=True)
    del img
    plain = mc.motion_correct_sum_fast_raw(raw, gain, field, ps, mean_zero=mean_zero)
    got = mc.motion_correct_sum_fast_raw(raw, gain, field, ps, mean_zero=mean_zero, dose_per_frame=dose,
                                         pre_exposure=pre, voltage=kv, return_plain_sum=True)
    assert torch.equal(plain, want_plain)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
@pytest.mark.parametrize("shape", [(5, 512, 1024), (3, 4092, 5760)])
def test_hot_pixels_fused(mc, dev, shape, dtype, monkeypatch):
    raw, gain = raw_movie(dev, *shape, dtype, seed=3 + shape[0], hot=True)
    field = rigid_field(dev, shape[0], 4.0, seed=9)
    img, want_counts = mc.condition_movie(raw, gain, hot_pixel_threshold=HOT, return_hot_counts=True)
    want_dw, want_plain = mc.motion_correct_sum_fast(img, field, 1.0, dose_per_frame=1.0, return_plain_sum=True)
    est = mc.estimate_global_motion(img, 1.0)
    want_est = mc.motion_correct_sum_fast(img, est, 1.0)
    del img
    assert int(want_counts.sum()) > 0
    refuse_conditioning(monkeypatch)  # the fused route really is taken
    dw, plain = mc.motion_correct_sum_fast_raw(raw, gain, field, 1.0, hot_pixel_threshold=HOT, dose_per_frame=1.0,
                                               return_plain_sum=True)
    assert range_err(dw, want_dw) <= 1e-5, range_err(dw, want_dw)
    assert range_err(plain, want_plain) <= 1e-5, range_err(plain, want_plain)
    f2, s2, counts = mc.motion_correct_raw_fast(raw, gain, 1.0, hot_pixel_threshold=HOT, return_hot_counts=True)
    assert torch.equal(counts.cpu(), want_counts.cpu())
    assert range_err(s2, want_est) <= 1e-5, range_err(s2, want_est)


@pytest.mark.parametrize("dtype,ps", [(torch.uint8, 1.0), (torch.int16, 1.3)])
def test_motion_correct_raw_fast(mc, dev, dtype, ps):
    t, h, w = 6, 1024, 1024
    raw, gain = raw_movie(dev, t, h, w, dtype, seed=21)
    field_raw, _ = mc.motion_correct_raw(raw, gain, ps)
    field, dw, plain = mc.motion_correct_raw_fast(raw, gain, ps, dose_per_frame=1.1, return_plain_sum=True)
    assert torch.equal(field, field_raw)
    field2, plain_only = mc.motion_correct_raw_fast(raw, gain, ps)
    assert torch.equal(field2, field_raw) and torch.equal(plain_only, plain)
    # the route at the top of the issue: condition -> estimate_global_motion -> correct_motion_fast -> sum / dose
    img = mc.condition_movie(raw, gain)
    efield = mc.estimate_global_motion(img, ps)
    assert torch.equal(efield, field)
    cor = mc.correct_motion_fast(img, efield.clone() / ps)  # the field in pixels (the example passes Angstrom)
    assert range_err(plain, cor.sum(0)) <= 2e-5
    assert range_err(dw, mc.dose_weighted_sum(cor, ps, 1.1)) <= 2e-5
    want = mc.motion_correct_sum_fast(img, efield, ps, dose_per_frame=1.1, return_plain_sum=True)
    assert torch.equal(dw, want[0]) and torch.equal(plain, want[1])


def test_no_fp32_movie_is_allocated(mc, dev):
    """40 x 4096^2 u8: the fused peak above the inputs is below the composition's by at least 1.5 fp32 movies."""
    t, h, w = 40, 4096, 4096
    raw, gain = raw_movie(dev, t, h, w, torch.uint8, seed=1)
    field = rigid_field(dev, t, 8.0, seed=3)
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

    def composition():
        img = mc.condition_movie(raw, gain)
        cor = mc.correct_motion_fast(img, field.clone())
        return cor.sum(0), mc.dose_weighted_sum(cor, 1.0, 1.0)

    fused = lambda: mc.motion_correct_sum_fast_raw(raw, gain, field, 1.0, dose_per_frame=1.0,  # noqa: E731
                                                   return_plain_sum=True)
    fused()  # plans and tables built once outside the measured calls
    composition()
    p_comp, p_fused = peak(composition), peak(fused)
    assert p_fused <= p_comp - 1.5 * 4 * t * h * w, (p_fused, p_comp)


@pytest.mark.parametrize("case", ["fp16", "fp32", "not_row_major", "polyphase", "hot_list_overflow"])
def test_fallbacks_are_exactly_the_conditioned_route(mc, dev, case, monkeypatch):
    shape = (4, 959, 928) if case == "not_row_major" else (4, 512, 1024)
    raw, gain = raw_movie(dev, *shape, torch.uint8, seed=7, hot=case == "hot_list_overflow")
    movie = {"fp16": raw.to(torch.float16), "fp32": raw.to(torch.float32)}.get(case, raw)
    hot = HOT if case == "hot_list_overflow" else None
    if case == "polyphase":
        monkeypatch.setattr(engine, "POLYPHASE_FOURIER_SHIFT", True)
    if case == "hot_list_overflow":
        monkeypatch.setattr(engine, "hot_list_capacity", lambda t, h, w: 4)
    field = rigid_field(dev, shape[0], 3.0, seed=5)
    dose = dict(dose_per_frame=1.2, pre_exposure=0.3, voltage=300.0)
    got = mc.motion_correct_sum_fast_raw(movie, gain, field, 1.1, hot_pixel_threshold=hot, return_plain_sum=True,
                                         **dose)
    img = mc.condition_movie(movie, gain, hot_pixel_threshold=hot)
    want = mc.motion_correct_sum_fast(img, field, 1.1, return_plain_sum=True, **dose)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    f, s = mc.motion_correct_raw_fast(movie, gain, 1.1, hot_pixel_threshold=hot)
    ef = mc.estimate_global_motion(img, 1.1)
    assert torch.equal(f, ef) and torch.equal(s, mc.motion_correct_sum_fast(img, ef, 1.1))
