"""Host-side checks of Fourier cropping (fourier_crop, fourier_crop_raw, motion_correct_raw_binned; mc_full_cols_crop):
the public signatures, argument validation before any device is touched, the C entry point's own checks (no launch),
and the float64 identities of the definition, which pin the expected-value helper the GPU tests use."""

import ctypes
import inspect

import pytest
import torch

from crop_reference import band_limited, crop64 as crop_ref  # noqa: F401  (tests/test_fourier_crop.py imports them here)
from kernel_harness import assert_entry_point
from torch_motion_correction_amd import _lib


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def test_public_entry_points_and_defaults():
    import torch_motion_correction_amd as mc

    for name in ("fourier_crop", "fourier_crop_raw", "motion_correct_raw_binned"):
        assert name in mc.__all__ and callable(getattr(mc, name))
    assert list(inspect.signature(mc.fourier_crop).parameters) == ["image", "binning", "device"]
    assert _defaults(mc.fourier_crop) == dict(binning=2, device=None)
    assert list(inspect.signature(mc.fourier_crop_raw).parameters) == [
        "movie", "gain", "binning", "mean_zero", "hot_pixel_threshold", "return_hot_counts", "device"]
    assert _defaults(mc.fourier_crop_raw) == dict(binning=2, mean_zero=True, hot_pixel_threshold=None,
                                                  return_hot_counts=False, device=None)
    params = list(inspect.signature(mc.motion_correct_raw_binned).parameters)
    assert params[:5] == ["movie", "gain", "pixel_spacing", "binning", "patch_sidelength"]
    assert set(params[5:]) == {"reference_frame", "b_factor", "frequency_range", "grid_type", "mean_zero",
                               "hot_pixel_threshold", "dose_per_frame", "pre_exposure", "voltage", "return_plain_sum",
                               "return_hot_counts", "device"}
    assert _defaults(mc.motion_correct_raw_binned) == dict(
        binning=2, patch_sidelength=None, reference_frame=None, b_factor=500, frequency_range=(300, 10),
        grid_type="catmull_rom", mean_zero=True, hot_pixel_threshold=None, dose_per_frame=None, pre_exposure=0.0,
        voltage=300.0, return_plain_sum=False, return_hot_counts=False, device=None)


BAD_HOT = [(dict(hot_pixel_threshold=0.0), "hot_pixel_threshold"),
           (dict(hot_pixel_threshold=float("inf")), "hot_pixel_threshold"),
           (dict(hot_pixel_threshold="ten"), "hot_pixel_threshold")]
BAD_DOSE = [(dict(dose_per_frame=-0.1), "dose_per_frame"), (dict(dose_per_frame=float("nan")), "dose_per_frame"),
            (dict(dose_per_frame="one"), "dose_per_frame"), (dict(return_plain_sum=True), "return_plain_sum")]
BAD_BINNING = [(dict(binning=1), "binning"), (dict(binning=4), "binning"), (dict(binning=2.5), "binning"),
               (dict(binning=None), "binning"), (dict(binning=True), "binning")]


@pytest.mark.parametrize("kw,match", BAD_BINNING)
def test_bad_binning_raises_before_any_device(kw, match):
    import torch_motion_correction_amd as mc

    raw = torch.zeros((3, 512, 1024), dtype=torch.uint8)  # CPU tensors: no device is ever needed
    with pytest.raises(ValueError, match=match):
        mc.fourier_crop(raw.float(), **kw)
    with pytest.raises(ValueError, match=match):
        mc.fourier_crop(raw[0].float(), **kw)
    with pytest.raises(ValueError, match=match):
        mc.fourier_crop_raw(raw, None, **kw)
    with pytest.raises(ValueError, match=match):
        mc.motion_correct_raw_binned(raw, None, 0.5, **kw)


@pytest.mark.parametrize("shape", [(3, 511, 1024), (3, 512, 1023), (2, 4091, 5761)])
def test_odd_sizes_raise_before_any_device(shape):
    import torch_motion_correction_amd as mc

    raw = torch.zeros(shape, dtype=torch.uint8)
    with pytest.raises(ValueError, match="even"):
        mc.fourier_crop(raw.float())
    with pytest.raises(ValueError, match="even"):
        mc.fourier_crop(raw[0].half())
    with pytest.raises(ValueError, match="even"):
        mc.fourier_crop_raw(raw, None)
    with pytest.raises(ValueError, match="even"):
        mc.motion_correct_raw_binned(raw, None, 0.5)


def test_bad_dimensions_and_gain_raise_before_any_device():
    import torch_motion_correction_amd as mc

    raw = torch.zeros((3, 512, 1024), dtype=torch.uint8)
    with pytest.raises(ValueError, match="image"):
        mc.fourier_crop(torch.zeros(512))
    with pytest.raises(ValueError, match="image"):
        mc.fourier_crop(torch.zeros(1, 2, 512, 512))
    with pytest.raises(ValueError, match="movie"):
        mc.fourier_crop_raw(raw[0], None)
    with pytest.raises(ValueError, match="movie"):
        mc.motion_correct_raw_binned(raw[0], None, 0.5)
    for gain in (torch.ones(512, 512), torch.ones(1024, 512), torch.ones(3, 512, 1024)):
        with pytest.raises(ValueError, match="gain"):
            mc.fourier_crop_raw(raw, gain)
        with pytest.raises(ValueError, match="gain"):
            mc.motion_correct_raw_binned(raw, gain, 0.5)


@pytest.mark.parametrize("kw,match", BAD_HOT)
def test_bad_hot_pixel_threshold_raises_before_any_device(kw, match):
    import torch_motion_correction_amd as mc

    raw = torch.zeros((3, 512, 1024), dtype=torch.uint8)
    with pytest.raises(ValueError, match=match):
        mc.fourier_crop_raw(raw, None, **kw)
    with pytest.raises(ValueError, match=match):
        mc.motion_correct_raw_binned(raw, None, 0.5, **kw)


@pytest.mark.parametrize("kw,match", BAD_DOSE)
def test_bad_dose_raises_before_any_device(kw, match):
    import torch_motion_correction_amd as mc

    raw = torch.zeros((3, 512, 1024), dtype=torch.uint8)
    with pytest.raises(ValueError, match=match):
        mc.motion_correct_raw_binned(raw, None, 0.5, **kw)


def test_patch_route_argument_rules():
    import torch_motion_correction_amd as mc

    raw = torch.zeros((3, 512, 1024), dtype=torch.uint8)
    with pytest.raises(ValueError, match="patch_sidelength"):
        mc.motion_correct_raw_binned(raw, None, 0.5, patch_sidelength=0)
    with pytest.raises(ValueError, match="return_plain_sum"):
        mc.motion_correct_raw_binned(raw, None, 0.5, patch_sidelength=256, dose_per_frame=1.0, return_plain_sum=True)


@pytest.mark.parametrize("shape", [(2, 4092, 5760), (2, 960, 928), (2, 256, 1024), (2, 512, 64), (2, 8192, 8192)])
def test_unsupported_even_sizes_name_the_supported_ones(shape):
    import torch_motion_correction_amd as mc

    raw = torch.zeros(shape, dtype=torch.uint8)
    for call in (lambda: mc.fourier_crop(raw[0].half()), lambda: mc.fourier_crop_raw(raw, None),
                 lambda: mc.motion_correct_raw_binned(raw, None, 0.5)):
        with pytest.raises(NotImplementedError, match="8184.*11520"):
            call()


def test_entry_point_is_declared_bound_and_exported():
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    assert_entry_point("mc_full_cols_crop", [vp, vp, vp, i32, i32, i32, i32, i32, vp])


def _p(i):
    return ctypes.c_void_p(0x100000 * (i + 1))


def test_cropping_column_pass_validates_on_the_host():
    """Fake pointers and a null stream: every call below must answer before it launches anything."""
    lib = _lib.load()

    def crop(S=_p(0), S2=_p(1), tw=_p(2), n=2, H=512, W=1024, pitch=None, pitch2=None):
        pitch = lib.mc_full_spectrum_pitch(W) if pitch is None else pitch
        pitch2 = lib.mc_full_spectrum_pitch(W // 2) if pitch2 is None else pitch2
        return lib.mc_full_cols_crop(S, S2, tw, n, H, W, pitch, pitch2, None)

    assert crop(S=None) == -1 and crop(S2=None) == -1 and crop(tw=None) == -1 and crop(n=0) == -1
    assert crop(H=256) == -2  # 128-point columns do not exist
    assert crop(H=4092) == -2  # 2046 = 2 3 11 31 is no column length
    assert crop(H=8192) == -2 and crop(H=1000) == -2
    assert crop(W=64) == -2  # 32-sample rows do not exist
    assert crop(W=5760) == -2  # 2880-sample rows (a 1440-point line) do not exist
    assert crop(W=1000) == -2 and crop(W=16384) == -2
    assert crop(H=511) == -2 and crop(H=513) == -2 and crop(W=1023) == -2 and crop(W=1025) == -2
    p2 = lib.mc_full_spectrum_pitch(512)
    assert crop(pitch2=p2 - 16) == -2 and crop(pitch2=p2 + 16) == -2 and crop(pitch2=257) == -2
    assert crop(pitch2=lib.mc_full_spectrum_pitch(1024)) == -2
    assert crop(pitch=512) == -2 and crop(pitch=lib.mc_full_spectrum_pitch(1024) + 1) == -2


# ---- the definition itself, in float64


SIZES = [(16, 24), (32, 20), (12, 8), (64, 40)]


@pytest.mark.parametrize("h,w", SIZES)
def test_band_limited_frames_are_decimated(h, w):
    x = band_limited(h, w, seed=h + w)
    y = crop_ref(x)
    assert y.shape == (h // 2, w // 2) and y.dtype == torch.float64
    assert float((y - 4 * x[::2, ::2]).abs().max()) <= 1e-13 * float(x.abs().max())


@pytest.mark.parametrize("h,w", SIZES)
def test_crop_is_linear_keeps_the_sum_and_a_zero_mean(h, w):
    g = torch.Generator().manual_seed(3 * h + w)
    x = torch.randn(5, h, w, generator=g, dtype=torch.float64) + 2.0
    y = crop_ref(x)
    assert y.shape == (5, h // 2, w // 2)
    scale = float(x.abs().max())
    assert float((crop_ref(x.sum(0)) - y.sum(0)).abs().max()) <= 1e-13 * 5 * scale
    assert torch.allclose(y.sum((1, 2)), x.sum((1, 2)), rtol=1e-13, atol=0)  # counts are kept
    z = x - x.mean((1, 2), keepdim=True)
    assert float(crop_ref(z).mean((1, 2)).abs().max()) <= 1e-15 * scale  # a mean of zero stays zero
    c = torch.full((h, w), 3.25, dtype=torch.float64)
    assert float((crop_ref(c) - 13.0).abs().max()) <= 1e-13  # a constant frame: 4 x the constant


def test_new_nyquist_row_comes_from_the_negative_side():
    """A pure ky = -h/4 wave (with a kx that makes it complex in the half spectrum) survives with its phase; taking
    the row from ky = +h/4 instead would conjugate it."""
    h, w = 16, 16
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    x = torch.cos(2 * torch.pi * (-(h // 4) * yy / h + 1 * xx / w) + 0.3)
    F = torch.fft.rfft2(x)
    want = torch.zeros(h // 2, w // 4 + 1, dtype=torch.complex128)
    want[h // 4, 1] = F[h - h // 4, 1]
    assert abs(F[h - h // 4, 1]) > 1.0 and abs(F[h // 4, 1]) < 1e-9
    assert torch.allclose(crop_ref(x), torch.fft.irfft2(want, s=(h // 2, w // 2)), atol=1e-13)
