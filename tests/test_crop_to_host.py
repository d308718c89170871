"""Host-side checks of Fourier cropping to a given size (fourier_crop_to, fourier_crop_to_raw, fourier_crop_shape,
fourier_crop_pixel_spacing; mc_full_cols_crop_to): the float64 definition the GPU tests compare against, pinned against
an independent dense statement and against the halving's; the shape helper; argument validation before any device is
touched; the C entry point's own checks (no launch); the public signatures."""

import ctypes
import inspect

import numpy as np
import pytest
import torch

import crop_reference as cr
import crop_to_reference as ct
from kernel_harness import assert_entry_point
from torch_motion_correction_amd import _lib


def _frames(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) + 2.0


# ---- the definition itself, in float64


@pytest.mark.parametrize("shape", [(8, 12), (6, 8)])
def test_crop_to64_is_the_dense_statement(shape):
    x = _frames((12, 16), seed=sum(shape))
    got = ct.crop_to64(x, shape)
    assert got.shape == shape and got.dtype == torch.float64
    assert float(np.abs(got.numpy() - ct.dense_crop_to64(x.numpy(), shape)).max()) <= 1e-13 * float(x.abs().max())


@pytest.mark.parametrize("h,w", [(16, 24), (32, 20), (12, 8), (64, 40)])
def test_crop_to64_at_half_size_is_crop64(h, w):
    x = _frames((3, h, w), seed=h + w)
    assert torch.equal(ct.crop_to64(x, (h // 2, w // 2)), cr.crop64(x))


@pytest.mark.parametrize("h,w,shape", [(12, 16, (8, 12)), (12, 16, (6, 8)), (24, 32, (18, 16)), (64, 40, (48, 10))])
def test_crop_to64_keeps_each_frames_sum(h, w, shape):
    x = _frames((5, h, w), seed=3 * h + w)
    y = ct.crop_to64(x, shape)
    assert y.shape == (5, *shape)
    assert torch.allclose(y.sum((1, 2)), x.sum((1, 2)), rtol=1e-13, atol=0)
    c = torch.full((h, w), 3.25, dtype=torch.float64)  # a constant frame: the constant times h w / (h2 w2)
    assert float((ct.crop_to64(c, shape) - 3.25 * h * w / (shape[0] * shape[1])).abs().max()) <= 1e-12


@pytest.mark.parametrize("h,w,shape", [(12, 16, (8, 12)), (12, 16, (6, 8)), (24, 32, (18, 16)), (36, 20, (24, 18))])
def test_a_band_limited_frame_comes_back_as_its_exact_resampling(h, w, shape):
    x = ct.band_limited_to(h, w, shape, seed=h + w)
    want = ct.resampled(x.numpy(), shape)
    assert float(np.abs(want).max()) > 0.1
    assert float(np.abs(ct.crop_to64(x, shape).numpy() - want).max()) <= 1e-12 * float(np.abs(want).max())


def test_new_nyquist_row_comes_from_the_negative_side():
    h, w, (h2, w2) = 12, 16, (8, 12)
    x = ct.impulse_frame(h, w, -(h2 // 2), 1, phase=0.3)
    F = torch.fft.rfft2(x)
    want = torch.zeros(h2, w2 // 2 + 1, dtype=torch.complex128)
    want[h2 // 2, 1] = F[h - h2 // 2, 1]
    assert abs(F[h - h2 // 2, 1]) > 1.0 and abs(F[h2 // 2, 1]) < 1e-9
    assert torch.allclose(ct.crop_to64(x, (h2, w2)), torch.fft.irfft2(want, s=(h2, w2)), atol=1e-13)


def test_the_bound_at_half_size_is_the_halvings():
    for h, w in ((512, 1024), (8184, 11520), (4096, 128)):
        a, b = ct.frame_bound(h, w, h // 2, w // 2, 3.0, 1.5, extra=1e-4), cr.frame_bound(h, w, 3.0, 1.5, extra=1e-4)
        for key in ("fwd", "l2", "cap"):
            assert a[key] == pytest.approx(b[key], rel=1e-12)
    for (t, h, w), (h2, w2) in ct.ROUTE_CASES + [ct.WHOLE_FRAME]:  # every line of the cases is one the bound prices
        c_fwd, c_inv = ct.frame_costs(h, w, h2, w2)
        assert 0 < c_inv < c_fwd + c_inv < 1e-3


# ---- the shape for a factor, the pixel spacing


@pytest.mark.parametrize("args,want", ct.SHAPES_FOR_FACTORS, ids=lambda v: "x".join(f"{a:g}" for a in v))
def test_fourier_crop_shape(args, want):
    import torch_motion_correction_amd as mc

    assert mc.fourier_crop_shape(*args) == want
    h, w, _ = args
    assert mc.engine.fourier_crop_to_supported(h, w, *want)


def test_an_unsupported_factor_lists_the_supported_ones():
    import torch_motion_correction_amd as mc

    with pytest.raises(NotImplementedError, match=r"factors 1\.5, 2, 3 for this size"):
        mc.fourier_crop_shape(8184, 11520, 2.5)
    with pytest.raises(NotImplementedError, match=r"factors 2 for this size"):
        mc.fourier_crop_shape(4092, 5760, 1.5)
    with pytest.raises(NotImplementedError, match=r"factors none for this size.*8184 -> 5456"):
        mc.fourier_crop_shape(4000, 4000, 2)
    with pytest.raises(NotImplementedError):
        mc.fourier_crop_shape(8184, 11520, 1.51)  # 0.66 % off on both axes
    assert mc.fourier_crop_shape(8184, 11520, 1.505) == (5456, 7680)  # 0.33 %
    for bad in (0.5, 0, -2, float("nan"), float("inf"), "two", None, True):
        with pytest.raises(ValueError, match="binning"):
            mc.fourier_crop_shape(8184, 11520, bad)


def test_fourier_crop_pixel_spacing():
    import torch_motion_correction_amd as mc

    assert mc.fourier_crop_pixel_spacing((8184, 11520), (5456, 7680), 0.5) == (0.75, 0.75)
    assert mc.fourier_crop_pixel_spacing((40, 4092, 5760), (40, 2046, 2880), 0.83) == pytest.approx((1.66, 1.66), rel=1e-15)
    assert mc.fourier_crop_pixel_spacing((512, 11520), (384, 3840), 1.0) == (512 / 384, 3.0)
    with pytest.raises(ValueError, match="positive"):
        mc.fourier_crop_pixel_spacing((512, 0), (384, 128), 1.0)


# ---- the public names and their argument rules


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def test_public_entry_points_and_defaults():
    import torch_motion_correction_amd as mc

    for name in ("fourier_crop_to", "fourier_crop_to_raw", "fourier_crop_shape", "fourier_crop_pixel_spacing"):
        assert name in mc.__all__ and callable(getattr(mc, name))
    assert list(inspect.signature(mc.fourier_crop_to).parameters) == ["image", "shape", "device"]
    assert _defaults(mc.fourier_crop_to) == dict(device=None)
    assert list(inspect.signature(mc.fourier_crop_to_raw).parameters) == [
        "movie", "gain", "shape", "mean_zero", "hot_pixel_threshold", "return_hot_counts", "device"]
    assert _defaults(mc.fourier_crop_to_raw) == dict(mean_zero=True, hot_pixel_threshold=None, return_hot_counts=False,
                                                     device=None)
    assert list(inspect.signature(mc.fourier_crop_shape).parameters) == ["h", "w", "binning"]
    assert _defaults(mc.fourier_crop_shape) == {}
    assert list(inspect.signature(mc.fourier_crop_pixel_spacing).parameters) == ["shape_in", "shape_out",
                                                                                 "pixel_spacing"]
    assert _defaults(mc.fourier_crop_pixel_spacing) == {}


RAW = torch.zeros((3, 512, 256), dtype=torch.uint8)  # CPU tensors: no device is ever needed
BAD_SHAPES = [((385, 128), "even"), ((384, 127), "even"), ((514, 128), "exceeds"), ((384, 258), "exceeds"),
              ((0, 128), "positive"), ((384, -2), "positive"), ((384,), "two integers"), ((384.0, 128), "two integers"),
              (None, "two integers")]


@pytest.mark.parametrize("shape,match", BAD_SHAPES, ids=[str(s) for s, _ in BAD_SHAPES])
def test_bad_shapes_raise_before_any_device(shape, match):
    import torch_motion_correction_amd as mc

    for call in (lambda: mc.fourier_crop_to(RAW.float(), shape), lambda: mc.fourier_crop_to(RAW[0].half(), shape),
                 lambda: mc.fourier_crop_to_raw(RAW, None, shape)):
        with pytest.raises(ValueError, match=match):
            call()


@pytest.mark.parametrize("shape", [(3, 511, 256), (3, 512, 255)])
def test_odd_frames_raise_before_any_device(shape):
    import torch_motion_correction_amd as mc

    raw = torch.zeros(shape, dtype=torch.uint8)
    with pytest.raises(ValueError, match="even"):
        mc.fourier_crop_to(raw.float(), (384, 128))
    with pytest.raises(ValueError, match="even"):
        mc.fourier_crop_to(raw[0].half(), (384, 128))
    with pytest.raises(ValueError, match="even"):
        mc.fourier_crop_to_raw(raw, None, (384, 128))


def test_bad_dimensions_gain_and_threshold_raise_before_any_device():
    import torch_motion_correction_amd as mc

    with pytest.raises(ValueError, match="image"):
        mc.fourier_crop_to(torch.zeros(512), (384, 128))
    with pytest.raises(ValueError, match="image"):
        mc.fourier_crop_to(torch.zeros(1, 2, 512, 256), (384, 128))
    with pytest.raises(ValueError, match="movie"):
        mc.fourier_crop_to_raw(RAW[0], None, (384, 128))
    for gain in (torch.ones(512, 512), torch.ones(256, 512), torch.ones(3, 512, 256)):
        with pytest.raises(ValueError, match="gain"):
            mc.fourier_crop_to_raw(RAW, gain, (384, 128))
    for thr in (0.0, float("inf"), "ten"):
        with pytest.raises(ValueError, match="hot_pixel_threshold"):
            mc.fourier_crop_to_raw(RAW, None, (384, 128), hot_pixel_threshold=thr)


@pytest.mark.parametrize("case", ct.UNSUPPORTED, ids=ct.case_id)
def test_unsupported_pairs_name_the_table(case):
    import torch_motion_correction_amd as mc

    shape, out_shape = case
    raw = torch.zeros(shape, dtype=torch.uint8)
    assert not mc.engine.fourier_crop_to_supported(*shape[1:], *out_shape)
    for call in (lambda: mc.fourier_crop_to(raw[0].half(), out_shape), lambda: mc.fourier_crop_to_raw(raw, None, out_shape)):
        with pytest.raises(NotImplementedError, match="8184 -> 5456.*7680"):
            call()


def test_the_supported_table():
    from torch_motion_correction_amd import engine

    for (t, h, w), (h2, w2) in ct.ROUTE_CASES + [ct.WHOLE_FRAME, ct.RAW]:
        assert engine.fourier_crop_to_supported(h, w, h2, w2)
    assert engine.fourier_crop_to_supported(4092, 5760, 2046, 2048)  # the axes are independent
    assert engine.fourier_crop_to_supported(512, 1024, 256, 512) and engine.fourier_crop_to_supported(8184, 11520, 4092, 5760)
    assert not engine.fourier_crop_to_supported(4092, 5760, 2046, 5762)
    assert not engine.fourier_crop_to_supported(512, 2880, 384, 2880)  # 2880 is no forward row length
    assert engine.fourier_crop_to_shapes(4096, 128) == [(2048, 64), (3072, 64), (3072, 128)]


# ---- the C entry point


def test_entry_point_is_declared_bound_and_exported():
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    assert_entry_point("mc_full_cols_crop_to", [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp],
                       source=("fourier_crop_to.hip", "fourier_crop_to", []))


def _p(i):
    return ctypes.c_void_p(0x100000 * (i + 1))


def test_cropping_column_pass_validates_on_the_host():
    """Fake pointers and a null stream: every call below must answer before it launches anything."""
    lib = _lib.load()

    def crop(S=_p(0), S2=_p(1), tw=_p(2), tw2=_p(3), n=2, H=512, W=256, H2=384, W2=128, pitch=None, pitch2=None):
        pitch = lib.mc_full_spectrum_pitch(W) if pitch is None else pitch
        pitch2 = lib.mc_full_spectrum_pitch(W2) if pitch2 is None else pitch2
        return lib.mc_full_cols_crop_to(S, S2, tw, tw2, n, H, W, H2, W2, pitch, pitch2, None)

    ARG, UNS = -1, -2
    assert crop(S=None) == ARG and crop(S2=None) == ARG and crop(tw=None) == ARG and crop(tw2=None) == ARG
    assert crop(n=0) == ARG and crop(n=-1) == ARG
    assert crop(S=None, H=1000) == ARG  # the arguments before the sizes, as in the other full-spectrum entries
    for H, H2 in ((512, 256), (512, 512), (512, 386), (1024, 768), (4096, 2048), (4092, 3072), (8184, 4092),
                  (8184, 5454), (384, 512), (2046, 4092), (4000, 2000), (512, 383), (512, 0), (0, 0)):
        assert crop(H=H, H2=H2) == UNS, (H, H2)  # a pair that is not in the table
    for W, W2 in ((256, 512), (256, 127), (256, 0), (255, 128), (4000, 128), (2880, 2880), (5760, 1440), (16384, 128),
                  (11520, 7682), (32, 32)):
        assert crop(W=W, W2=W2) == UNS, (W, W2)
    p2 = lib.mc_full_spectrum_pitch(128)
    assert crop(pitch2=p2 - 16) == UNS and crop(pitch2=p2 + 16) == UNS and crop(pitch2=65) == UNS  # a wrong pitch2
    assert crop(pitch2=lib.mc_full_spectrum_pitch(256)) == UNS
    assert crop(pitch=128) == UNS  # too narrow for W/2 + 1 bins
    assert crop(pitch=lib.mc_full_spectrum_pitch(256) + 1) == UNS and crop(pitch=lib.mc_full_spectrum_pitch(256) + 8) == UNS


def test_inverse_row_pass_takes_the_cropped_sizes_and_no_others():
    """mc_full_rows_inverse: the four new lines and the five new heights answer a null pointer with MC_ERR_ARG and a
    misaligned output with MC_ERR_UNSUPPORTED like every size (no launch); the forward passes and the shifting column
    pass still refuse them, and the halving's column pass still refuses 5760 columns."""
    lib = _lib.load()
    A, B, C_, D = (_p(i) for i in range(4))
    odd = ctypes.c_void_p(0x200004)
    for h2, w2 in ((384, 2880), (2046, 3072), (2728, 3840), (5456, 7680), (3072, 64), (256, 7680)):
        pitch2 = lib.mc_full_spectrum_pitch(w2)
        assert lib.mc_full_rows_inverse(A, None, C_, w2, D, 1, h2, w2, pitch2, None) == -1
        assert lib.mc_full_rows_inverse(A, odd, C_, w2, D, 1, h2, w2, pitch2, None) == -2
        assert lib.mc_full_rows_inverse(A, B, C_, w2, D, 1, h2, w2, pitch2 + 1, None) == -2
    for h2, w2 in ((384, 2880), (256, 3072), (384, 64)):
        pitch2 = lib.mc_full_spectrum_pitch(w2)
        assert lib.mc_full_rows_forward(A, B, w2, C_, D, 1, h2, w2, pitch2, None) == -2
        assert lib.mc_full_cols_shift(A, B, C_, 1.0, 1, h2, w2, pitch2, None) == -2
    for h2, w2 in ((386, 2880), (384, 2882), (384, 1440), (1364, 64)):
        assert lib.mc_full_rows_inverse(A, B, C_, w2, D, 1, h2, w2, lib.mc_full_spectrum_pitch(w2), None) == -2
    assert lib.mc_full_cols_crop(A, B, C_, 2, 512, 5760, lib.mc_full_spectrum_pitch(5760),
                                 lib.mc_full_spectrum_pitch(2880), None) == -2
