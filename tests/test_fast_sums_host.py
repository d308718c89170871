"""Host-side checks of the fused Fourier-shift sums (motion_correct_sum_fast, motion_correct_sum_fast_raw,
motion_correct_raw_fast; mc_full_rows_forward_raw, mc_full_rows_hot_correct, mc_full_cols_shift_sum[_cm]): the public
signatures, argument validation before any device is touched, the C entry points' own checks (no launch), and a
float64 check of the two identities the fused route rests on."""

import ctypes
import inspect
import math

import pytest
import torch

from kernel_harness import assert_entry_point
from torch_motion_correction_amd import _lib

U8, I16 = 0, 1


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def test_public_entry_points_and_defaults():
    import torch_motion_correction_amd as mc

    for name in ("motion_correct_sum_fast", "motion_correct_sum_fast_raw", "motion_correct_raw_fast"):
        assert name in mc.__all__
    assert list(inspect.signature(mc.motion_correct_sum_fast).parameters) == [
        "image", "deformation_grid", "pixel_spacing", "dose_per_frame", "pre_exposure", "voltage", "return_plain_sum",
        "device"]
    assert _defaults(mc.motion_correct_sum_fast) == dict(dose_per_frame=None, pre_exposure=0.0, voltage=300.0,
                                                         return_plain_sum=False, device=None)
    assert list(inspect.signature(mc.motion_correct_sum_fast_raw).parameters) == [
        "movie", "gain", "deformation_grid", "pixel_spacing", "mean_zero", "hot_pixel_threshold", "dose_per_frame",
        "pre_exposure", "voltage", "return_plain_sum", "device"]
    assert _defaults(mc.motion_correct_sum_fast_raw) == dict(mean_zero=True, hot_pixel_threshold=None,
                                                             dose_per_frame=None, pre_exposure=0.0, voltage=300.0,
                                                             return_plain_sum=False, device=None)
    assert list(inspect.signature(mc.motion_correct_raw_fast).parameters) == [
        "movie", "gain", "pixel_spacing", "reference_frame", "b_factor", "frequency_range", "mean_zero",
        "hot_pixel_threshold", "dose_per_frame", "pre_exposure", "voltage", "return_plain_sum", "return_hot_counts",
        "device"]
    assert _defaults(mc.motion_correct_raw_fast) == dict(
        reference_frame=None, b_factor=500, frequency_range=(300, 10), mean_zero=True, hot_pixel_threshold=None,
        dose_per_frame=None, pre_exposure=0.0, voltage=300.0, return_plain_sum=False, return_hot_counts=False,
        device=None)


def _movie_and_field(t=3, h=64, w=64, gh=1, gw=1, dtype=torch.uint8):
    return torch.zeros((t, h, w), dtype=dtype), torch.zeros((2, t, gh, gw))


BAD = [(dict(dose_per_frame=-0.1), "dose_per_frame"), (dict(dose_per_frame=float("nan")), "dose_per_frame"),
       (dict(dose_per_frame="one"), "dose_per_frame"), (dict(return_plain_sum=True), "return_plain_sum")]
BAD_HOT = [(dict(hot_pixel_threshold=0.0), "hot_pixel_threshold"),
           (dict(hot_pixel_threshold=float("inf")), "hot_pixel_threshold"),
           (dict(hot_pixel_threshold="ten"), "hot_pixel_threshold")]


@pytest.mark.parametrize("kw,match", BAD)
def test_fp32_bad_arguments_raise_before_any_device(kw, match):
    import torch_motion_correction_amd as mc

    img, field = _movie_and_field(dtype=torch.float32)  # CPU tensors: no device is ever needed
    with pytest.raises(ValueError, match=match):
        mc.motion_correct_sum_fast(img, field, 1.0, **kw)


@pytest.mark.parametrize("kw,match", BAD + BAD_HOT)
def test_raw_bad_arguments_raise_before_any_device(kw, match):
    import torch_motion_correction_amd as mc

    raw, field = _movie_and_field()
    with pytest.raises(ValueError, match=match):
        mc.motion_correct_sum_fast_raw(raw, None, field, 1.0, **kw)
    with pytest.raises(ValueError, match=match):
        mc.motion_correct_raw_fast(raw, None, 1.0, **kw)


@pytest.mark.parametrize("shape,match", [((2, 3, 2, 2), "single patch"), ((2, 3, 1, 4), "single patch"),
                                         ((3, 1, 1), "deformation_grid"), ((1, 3, 1, 1), "deformation_grid"),
                                         ((2, 0, 1, 1), "deformation_grid"), ((2, 4, 1, 1), "time points"),
                                         ((2, 3, 1, 1, 1), "deformation_grid")])
def test_bad_fields_raise_before_any_device(shape, match):
    import torch_motion_correction_amd as mc

    raw, _ = _movie_and_field()
    with pytest.raises(ValueError, match=match):
        mc.motion_correct_sum_fast(raw.float(), torch.zeros(shape), 1.0)
    with pytest.raises(ValueError, match=match):
        mc.motion_correct_sum_fast_raw(raw, None, torch.zeros(shape), 1.0, dose_per_frame=1.0)


def test_non_rigid_field_gets_correct_motion_fast_message():
    import torch_motion_correction_amd as mc

    img = torch.zeros((3, 64, 64))
    with pytest.raises(ValueError) as ours:
        mc.motion_correct_sum_fast(img, torch.zeros((2, 3, 2, 2)), 1.0)
    import oracle

    with pytest.raises(ValueError) as theirs:
        oracle.correct_motion_fast(img, torch.zeros((2, 3, 2, 2)))
    assert str(ours.value) == str(theirs.value)


def test_gain_of_another_shape_raises_before_any_device():
    import torch_motion_correction_amd as mc

    raw, field = _movie_and_field()
    with pytest.raises(ValueError, match="gain"):
        mc.motion_correct_sum_fast_raw(raw, torch.ones(64, 32), field, 1.0)
    with pytest.raises(ValueError, match="gain"):
        mc.motion_correct_raw_fast(raw, torch.ones(32, 64), 1.0)


NEW = ("mc_full_rows_forward_raw", "mc_full_rows_hot_correct", "mc_full_cols_shift_sum", "mc_full_cols_shift_sum_cm")


def test_new_entry_points_are_declared_and_bound():
    for name in NEW:
        assert_entry_point(name)
    assert _lib.SIGNATURES["mc_full_cols_shift_sum"] == _lib.SIGNATURES["mc_full_cols_shift_sum_cm"]


def _p(i):
    return ctypes.c_void_p(0x100000 * (i + 1))


def test_raw_row_pass_validates_on_the_host():
    lib = _lib.load()

    def rows(raw=_p(0), kind=U8, gain=_p(1), mu=_p(2), off=_p(3), S=_p(4), tw=_p(5), n=2, H=512, W=1024, pitch=None):
        pitch = lib.mc_full_spectrum_pitch(W) if pitch is None else pitch
        return lib.mc_full_rows_forward_raw(raw, kind, gain, mu, off, S, tw, n, H, W, pitch, None)

    assert rows(raw=None) == -1 and rows(gain=None) == -1 and rows(mu=None) == -1 and rows(off=None) == -1
    assert rows(S=None) == -1 and rows(tw=None) == -1 and rows(n=0) == -1
    assert rows(kind=2) == -2 and rows(kind=3) == -2  # fp16 / fp32: condition the movie first
    assert rows(W=1000) == -2 and rows(H=300) == -2 and rows(W=1024, pitch=520) == -2
    assert rows(kind=I16, raw=ctypes.c_void_p(0x100002)) == -2  # i16 pairs: 4-byte aligned
    assert rows(raw=ctypes.c_void_p(0x100001)) == -2  # u8 pairs: 2-byte aligned
    assert rows(gain=ctypes.c_void_p(0x200004)) == -2  # gain pairs: 8-byte aligned


def test_hot_correction_validates_on_the_host():
    lib = _lib.load()
    pitch = lib.mc_full_spectrum_pitch(1024)

    def hot(keys=_p(0), rv=_p(1), n=5, f0=0, nj=2, H=512, W=1024, S=_p(2), pitch=pitch):
        return lib.mc_full_rows_hot_correct(keys, rv, n, f0, nj, H, W, S, pitch, None)

    assert hot(S=None) == -1 and hot(keys=None) == -1 and hot(rv=None) == -1
    assert hot(n=-1) == -1 and hot(f0=-1) == -1 and hot(nj=0) == -1
    assert hot(W=1000) == -2 and hot(pitch=520) == -2
    assert hot(n=0, keys=None, rv=None) == 0  # nothing to correct: no launch


def test_shift_sum_validates_on_the_host():
    lib = _lib.load()

    def run(S=_p(0), shifts=_p(1), n=2, f0=0, total=2, A=_p(2), P=_p(3), tw=_p(4), H=512, W=1024, ps=1.0, dose=1.0,
            cm=False):
        pitch = lib.mc_full_spectrum_pitch(W)
        fn = lib.mc_full_cols_shift_sum_cm if cm else lib.mc_full_cols_shift_sum
        return fn(S, shifts, n, f0, total, A, P, tw, H, W, pitch, ps, 0.0, dose, 300.0, 1, 1, 1.0, None)

    assert run(S=None) == -1 and run(shifts=None) == -1 and run(tw=None) == -1
    assert run(A=None, P=None) == -1  # at least one sum
    assert run(n=0) == -1 and run(f0=-1) == -1 and run(total=1) == -1
    assert run(ps=0.0) == -1 and run(dose=-1.0) == -1 and run(dose=float("nan")) == -1
    assert run(W=1000) == -2 and run(H=300) == -2
    assert run(cm=True) == -2  # the column-major feed: 4096 / 4092 / 8184 rows only
    # shifts=None: no phase ramp, the exposure-weighted sum alone (P set: -1); the other rules hold as they are
    assert run(shifts=None, A=None) == -1
    for cm in (False, True):
        def bare(**kw):
            return run(shifts=None, P=None, cm=cm, **kw)

        assert bare(S=None) == -1 and bare(tw=None) == -1 and bare(A=None) == -1
        assert bare(n=0) == -1 and bare(f0=-1) == -1 and bare(total=1) == -1
        assert bare(ps=0.0) == -1 and bare(dose=-1.0) == -1 and bare(dose=float("nan")) == -1
        assert bare(W=1000) == -2 and bare(H=300) == -2
    assert run(shifts=None, P=None, cm=True) == -2  # the column-major feed: 4096 / 4092 / 8184 rows only


def _ramp(h, w, sy, sx):
    fy = torch.fft.fftfreq(h, dtype=torch.float64)[:, None]
    fx = torch.fft.rfftfreq(w, dtype=torch.float64)[None, :]
    return torch.exp(-2j * math.pi * (fy * sy + fx * sx))


@pytest.mark.parametrize("h,w", [(16, 16), (15, 16), (16, 15), (15, 17), (12, 10)])
def test_linearity_identities_in_float64(h, w):
    """sum_f irfft2(R_f X_f) = irfft2(sum_f R_f X_f), and dose weighting the shifted frames
    (rfft2 -> q_f -> irfft2, summed) equals irfft2(sum_f q_f R_f X_f): q_f real and even in ky, irfft2 ignores
    what rfft2(irfft2(.)) projects away."""
    g = torch.Generator().manual_seed(h * 100 + w)
    t = 4
    x = torch.randn(t, h, w, generator=g, dtype=torch.float64)
    shifts = 6 * torch.rand(t, 2, generator=g, dtype=torch.float64) - 3
    X = torch.fft.rfft2(x)
    R = torch.stack([_ramp(h, w, float(s[0]), float(s[1])) for s in shifts])
    shifted = torch.fft.irfft2(R * X, s=(h, w))
    assert torch.allclose(shifted.sum(0), torch.fft.irfft2((R * X).sum(0), s=(h, w)), atol=1e-12)
    fy = torch.fft.fftfreq(h, dtype=torch.float64)[:, None]
    fx = torch.fft.rfftfreq(w, dtype=torch.float64)[None, :]
    k = torch.sqrt(fy * fy + fx * fx)
    q = torch.stack([torch.exp(-(0.5 + f) * 3.0 * k) for f in range(t)])  # real, even in ky
    norm = torch.sqrt((q * q).sum(0))
    dw = torch.fft.irfft2((q * torch.fft.rfft2(shifted)).sum(0) / norm, s=(h, w))
    fused = torch.fft.irfft2((q * R * X).sum(0) / norm, s=(h, w))
    assert torch.allclose(dw, fused, atol=1e-12)
