"""Fourier cropping (2x binning) on the GPU: fourier_crop, fourier_crop_raw and motion_correct_raw_binned against the
float64 CPU formula of the definition (tests/test_fourier_crop_host.py pins it) and against the compositions they are
defined as.  Errors are range_err of tests/test_raw_fast_sums.py: max |a - b| / range of b.

Largest range_err observed (MI355X, one run): see DESIGN.md section 4, "Fourier crop"."""

import pytest
import torch

import oracle
from test_fourier_crop_host import band_limited, crop_ref
from test_raw_fast_sums import raw_movie, range_err, refuse_conditioning
from torch_motion_correction_amd import engine

pytestmark = pytest.mark.gpu

HOT = 10.0
TOL = 1e-5


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def frames_fp32(t, h, w, seed):
    """A smooth texture + white noise + an offset (so the DC bin, the kept band and the discarded band all carry
    signal), made on the CPU."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(t, h, w, generator=g)
    x = x + 2.0 * (torch.roll(x, 1, 1) + torch.roll(x, 1, 2) + torch.roll(x, (2, 3), (1, 2))) + 3.0
    return x


SHAPES = [(5, 512, 1024), (3, 4096, 256), (2, 2048, 8192), (2, 4096, 4096), (2, 8184, 11520)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fourier_crop_matches_the_float64_formula(mc, dev, shape):
    t, h, w = shape
    x = frames_fp32(t, h, w, seed=h + w)
    xd = x.to(dev)
    keep = xd.clone()
    y = mc.fourier_crop(xd)
    assert y.shape == (t, h // 2, w // 2) and y.dtype == torch.float32 and y.device == xd.device
    assert torch.equal(xd, keep)  # the input is not modified
    err = range_err(y, crop_ref(x))
    print(f"fourier_crop {shape}: range_err {err:.3e}")
    assert err <= TOL, err


def test_a_single_image_and_the_device_rule(mc, dev):
    x = frames_fp32(1, 1024, 2048, seed=5)[0]
    want = crop_ref(x)
    y = mc.fourier_crop(x.to(dev))
    assert y.shape == (512, 1024) and y.dtype == torch.float32 and y.device.type == "cuda"
    err = range_err(y, want)
    print(f"fourier_crop 2-D image: range_err {err:.3e}")
    assert err <= TOL, err
    y_cpu = mc.fourier_crop(x)  # a CPU image comes back on the CPU, computed on the GPU
    assert y_cpu.device.type == "cpu" and torch.equal(y_cpu, y.cpu())
    assert mc.fourier_crop(x, device=dev).device.type == "cuda"
    y16 = mc.fourier_crop(x.half().to(dev))  # fp16 is widened, the result is fp32
    assert y16.dtype == torch.float32 and torch.equal(y16, mc.fourier_crop(x.half().float().to(dev)))


@pytest.mark.parametrize("shape", [(2, 512, 1024), (2, 4096, 4096), (1, 8184, 11520)],
                         ids=lambda s: "x".join(map(str, s)))
def test_band_limited_frames_are_decimated(mc, dev, shape):
    t, h, w = shape
    x = band_limited(h, w, seed=h, t=t).float()
    y = mc.fourier_crop(x.to(dev))
    err = range_err(y, 4 * x[:, ::2, ::2])
    print(f"fourier_crop band-limited {shape}: range_err {err:.3e}")
    assert err <= TOL, err


def test_a_constant_frame_gives_four_times_the_constant(mc, dev):
    x = torch.full((2, 1024, 512), 3.25, device=dev)
    y = mc.fourier_crop(x)
    assert float((y - 13.0).abs().max()) <= TOL * 13.0


# (dtype, gain, mean_zero)
CASES = {"u8": (torch.uint8, True, True), "i16": (torch.int16, True, True), "no_gain": (torch.uint8, False, True),
         "not_mean_zero": (torch.int16, True, False)}


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("shape", [(5, 512, 1024), (3, 8184, 11520)], ids=lambda s: "x".join(map(str, s)))
def test_raw_without_hot_pixels_equals_the_conditioned_route(mc, dev, shape, case):
    dtype, with_gain, mean_zero = CASES[case]
    raw, gain = raw_movie(dev, *shape, dtype, seed=sum(shape))
    gain = gain if with_gain else None
    want = mc.fourier_crop(mc.condition_movie(raw, gain, mean_zero=mean_zero))
    got = mc.fourier_crop_raw(raw, gain, mean_zero=mean_zero)
    assert got.dtype == torch.float32 and got.shape == (shape[0], shape[1] // 2, shape[2] // 2)
    assert torch.equal(got, want)
    got2, counts = mc.fourier_crop_raw(raw, gain, mean_zero=mean_zero, return_hot_counts=True)
    assert torch.equal(got2, want) and counts.dtype == torch.int32 and not counts.any()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
@pytest.mark.parametrize("shape", [(5, 512, 1024), (3, 8184, 11520)], ids=lambda s: "x".join(map(str, s)))
def test_raw_hot_pixels_fused(mc, dev, shape, dtype, monkeypatch):
    raw, gain = raw_movie(dev, *shape, dtype, seed=3 + shape[0], hot=True)
    img, want_counts = mc.condition_movie(raw, gain, hot_pixel_threshold=HOT, return_hot_counts=True)
    want = mc.fourier_crop(img)
    del img
    assert int(want_counts.sum()) > 0
    refuse_conditioning(monkeypatch)  # the fused route really is taken
    got, counts = mc.fourier_crop_raw(raw, gain, hot_pixel_threshold=HOT, return_hot_counts=True)
    assert torch.equal(counts, want_counts)
    err = range_err(got, want)
    print(f"fourier_crop_raw hot pixels {shape} {dtype}: range_err {err:.3e}")
    assert err <= TOL, err


@pytest.mark.parametrize("case", ["fp16", "fp32", "hot_list_overflow"])
def test_fallbacks_are_exactly_the_composition(mc, dev, case, monkeypatch):
    shape = (4, 512, 1024)
    raw, gain = raw_movie(dev, *shape, torch.uint8, seed=7, hot=case == "hot_list_overflow")
    movie = {"fp16": raw.to(torch.float16), "fp32": raw.to(torch.float32)}.get(case, raw)
    hot = HOT if case == "hot_list_overflow" else None
    if case == "hot_list_overflow":
        monkeypatch.setattr(engine, "hot_list_capacity", lambda t, h, w: 4)
    got, counts = mc.fourier_crop_raw(movie, gain, hot_pixel_threshold=hot, return_hot_counts=True)
    img, want_counts = mc.condition_movie(movie, gain, hot_pixel_threshold=hot, return_hot_counts=True)
    assert torch.equal(got, mc.fourier_crop(img)) and torch.equal(counts, want_counts)
    f, s = mc.motion_correct_raw_binned(movie, gain, 0.5, hot_pixel_threshold=hot)
    binned = mc.fourier_crop(img)
    ef = mc.estimate_global_motion(binned, 1.0)
    assert torch.equal(f, ef) and torch.equal(s, mc.motion_correct_sum_fast(binned, ef, 1.0))


def test_no_full_size_fp32_movie_is_allocated(mc, dev):
    """40 x 4096^2 u8: the composition holds exactly one full-size fp32 movie more than the fused route; the fused
    peak above the inputs must sit at least 0.9 of one below the composition's."""
    t, h, w = 40, 4096, 4096
    raw, gain = raw_movie(dev, t, h, w, torch.uint8, seed=1)
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

    composition = lambda: mc.fourier_crop(mc.condition_movie(raw, gain))  # noqa: E731
    fused = lambda: mc.fourier_crop_raw(raw, gain)  # noqa: E731
    fused()  # plans and tables built once outside the measured calls
    composition()
    p_comp, p_fused = peak(composition), peak(fused)
    print(f"peak above the inputs: composition {p_comp / 2**30:.2f} GiB, fused {p_fused / 2**30:.2f} GiB")
    assert p_fused <= p_comp - 0.9 * 4 * t * h * w, (p_fused, p_comp)


def drift_u8(dev, t, h, w, seed):
    """A u8 movie of one texture cropped at integer drifts of EVEN pixel counts (so the binned movie drifts by
    whole binned pixels) + noise; returns (raw, gain, dy, dx) with the drifts in full-size pixels."""
    g = torch.Generator().manual_seed(seed)
    pad = 32
    base = torch.randn(h + 2 * pad, w + 2 * pad, generator=g)
    base = base + torch.roll(base, 1, 0) + torch.roll(base, 1, 1) + torch.roll(base, (1, 1), (0, 1))
    dy = 2 * torch.round(torch.linspace(-4, 5, t)).long()
    dx = 2 * torch.round(torch.linspace(3, -3, t)).long()
    frames = [base[pad - dy[f]: pad - dy[f] + h, pad - dx[f]: pad - dx[f] + w] + 0.5 * torch.randn(h, w, generator=g)
              for f in range(t)]
    raw = (20 * torch.stack(frames) + 120).round().clamp(0, 255).to(torch.uint8)
    gain = 1.0 + 0.05 * (2 * torch.rand(h, w, generator=g) - 1)
    return raw.to(dev), gain.to(dev), dy, dx


@pytest.mark.parametrize("dose", [None, 1.1])
def test_binned_whole_image_route_is_the_composition(mc, dev, dose):
    ps = 0.42
    raw, gain = raw_movie(dev, 6, 2048, 2048, torch.uint8, seed=21)
    binned = mc.fourier_crop_raw(raw, gain)
    field = mc.estimate_global_motion(binned, 2 * ps)
    if dose is None:
        got = mc.motion_correct_raw_binned(raw, gain, ps)
        want = (field, mc.motion_correct_sum_fast(binned, field, 2 * ps))
    else:
        got = mc.motion_correct_raw_binned(raw, gain, ps, dose_per_frame=dose, pre_exposure=0.5, voltage=200.0,
                                           return_plain_sum=True, return_hot_counts=True)
        want = (field, *mc.motion_correct_sum_fast(binned, field, 2 * ps, dose_per_frame=dose, pre_exposure=0.5,
                                                   voltage=200.0, return_plain_sum=True),
                torch.zeros(6, dtype=torch.int32, device=dev))
        only = mc.motion_correct_raw_binned(raw, gain, ps, dose_per_frame=dose, pre_exposure=0.5, voltage=200.0)
        assert len(only) == 2 and torch.equal(only[1], want[1])
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and torch.equal(a, b)
    assert got[0].shape == (2, 6, 1, 1) and got[1].shape == (1024, 1024)


def test_binned_patch_route_is_the_composition(mc, dev):
    ps = 0.5
    raw, gain = raw_movie(dev, 6, 4096, 4096, torch.uint8, seed=4)
    binned = mc.fourier_crop_raw(raw, gain)
    field, centers = mc.estimate_motion_cross_correlation_patches(binned, 2 * ps, patch_sidelength=1024)
    got = mc.motion_correct_raw_binned(raw, gain, ps, patch_sidelength=1024)
    assert len(got) == 3
    assert torch.equal(got[0], field) and torch.equal(got[1], centers)
    assert torch.equal(got[2], mc.motion_correct_sum(binned, field, 2 * ps))
    assert got[2].shape == (2048, 2048) and field.shape[-2:] != (1, 1)
    dw = mc.motion_correct_raw_binned(raw, gain, ps, patch_sidelength=1024, dose_per_frame=1.0)
    assert torch.equal(dw[0], field)
    assert torch.equal(dw[2], mc.motion_correct_sum(binned, field, 2 * ps, dose_per_frame=1.0))


def test_binned_field_agrees_with_the_reference_estimator_on_the_float64_crop(mc, dev):
    """The reference's semantics: its whole-image estimator, on the CPU, on the float64-formula crop of the
    conditioned movie, gives the field motion_correct_raw_binned returns (in binned pixels) to 1e-4."""
    ps = 0.75
    raw, gain, dy, dx = drift_u8(dev, 8, 1024, 1024, seed=11)
    field, total = mc.motion_correct_raw_binned(raw, gain, ps)
    assert field.shape == (2, 8, 1, 1) and total.shape == (512, 512)
    cond = mc.condition_movie(raw, gain).cpu()
    ref = oracle.estimate_global_motion(crop_ref(cond).float(), 1.0)
    got = field.cpu() / (2 * ps)
    print("binned shifts (px):", got[:, :, 0, 0].tolist(), "half the planted drift:", (dy / 2).tolist(),
          (dx / 2).tolist())
    assert float((got - ref).abs().max()) <= 1e-4, (got.flatten().tolist(), ref.flatten().tolist())


@pytest.mark.parametrize("shape", [(2, 4092, 5760), (2, 960, 928)])
def test_unsupported_even_sizes_raise_before_any_launch(mc, dev, shape, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a kernel was about to be launched")

    monkeypatch.setattr(engine, "_rows_forward", refuse)
    monkeypatch.setattr(engine, "_raw_rows_forward", refuse)
    monkeypatch.setattr(engine.RawMovie, "__init__", refuse)
    refuse_conditioning(monkeypatch)
    raw = torch.zeros(shape, dtype=torch.uint8, device=dev)
    with pytest.raises(NotImplementedError, match="8184.*11520"):
        mc.fourier_crop(raw.float())
    with pytest.raises(NotImplementedError, match="8184.*11520"):
        mc.fourier_crop_raw(raw, None)
    with pytest.raises(NotImplementedError, match="8184.*11520"):
        mc.motion_correct_raw_binned(raw, None, 1.0)
    with pytest.raises(engine._lib.McorrUnsupported):
        engine.fourier_crop(raw.float())
