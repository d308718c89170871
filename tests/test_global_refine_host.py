"""Iterative sub-pixel whole-frame alignment, without a GPU: the float64 restatement (tests/global_refine_reference.py)
recovers planted fractional drifts that the integer estimate cannot, converges as the damped update promises and keeps
its guards; the public functions check their arguments before any device is touched."""

import numpy as np
import pytest
import torch

import global_refine_reference as gr
import torch_motion_correction_amd as mc
from torch_motion_correction_amd import engine


@pytest.fixture(scope="module")
def planted():
    """(8, 256, 256), drifts linspace(-3.3, 4.6) / (2.7, -1.9), white noise of 0.5 sigma: spectra and truth."""
    t, h, w = 8, 256, 256
    dy, dx = np.linspace(-3.3, 4.6, t), np.linspace(2.7, -1.9, t)
    movie, _ = gr.planted_movie(t, h, w, dy, dx, noise=0.5, seed=1)
    ref = t // 2
    truth = np.stack([dy - dy[ref], dx - dx[ref]], axis=1)
    return gr.filtered_spectra(movie, 1.0), (h, w), truth


def test_restatement_recovers_the_planted_drift(planted):
    S, shape, truth = planted
    s, hist, _ = gr.refine_shifts(S, shape, max_iterations=5, threshold=0.0)
    err = float(np.abs(s - truth).max())
    int_err = float(np.abs(gr.integer_shifts(S, shape, len(S) // 2) - truth).max())
    print(f"refined {err:.4f} px, integer {int_err:.4f} px, max|r| {hist}")
    assert len(hist) == 5
    assert err <= 0.1, err
    assert int_err >= 0.3, int_err


@pytest.mark.parametrize("t", [2, 3, 8])
def test_restatement_converges(t):
    """max |r| falls monotonically and is below 0.01 px within 4 iterations."""
    h = w = 128
    movie, _ = gr.planted_movie(t, h, w, np.linspace(-3.3, 4.6, t), np.linspace(2.7, -1.9, t), noise=0.25, seed=t)
    _, hist, _ = gr.refine_shifts(gr.filtered_spectra(movie, 1.0), (h, w), max_iterations=4, threshold=0.0)
    print(t, hist)
    assert all(b < a for a, b in zip(hist, hist[1:])), hist
    assert min(hist) < 0.01 and hist[-1] < 0.01, hist


def test_undamped_update_oscillates_for_two_frames():
    """Why the factor (t - 1)/t: with t = 2 each frame sees the other's whole error, an undamped update overshoots
    by the full residual and max |r| never falls."""
    movie, _ = gr.planted_movie(2, 128, 128, [0.0, 0.4], [0.0, -0.3], noise=0.25, seed=5)
    S = gr.filtered_spectra(movie, 1.0)
    _, damped, _ = gr.refine_shifts(S, (128, 128), max_iterations=4, threshold=0.0)
    _, undamped, _ = gr.refine_shifts(S, (128, 128), max_iterations=4, threshold=0.0, damping=1.0)
    assert damped[-1] < 0.01 < undamped[-1], (damped, undamped)


def test_stops_at_the_threshold(planted):
    S, shape, _ = planted
    _, hist, _ = gr.refine_shifts(S, shape, max_iterations=10, threshold=0.01)
    assert 1 <= len(hist) < 10 and hist[-1] < 0.01 and all(x >= 0.01 for x in hist[:-1]), hist


def test_parabola_guards_and_the_circular_neighbourhood():
    assert gr.parabola_offset(1.0, 3.0, 1.0) == 0.0  # equal outer samples: the axis is skipped
    assert gr.parabola_offset(1.0, 3.0, 2.0) == pytest.approx(0.5 * (1 - 2) / (1 - 6 + 2))
    cc = np.zeros((8, 10))
    cc[0, 0], cc[7, 0], cc[1, 0], cc[0, 9], cc[0, 1] = 4.0, 1.0, 2.0, 3.0, 3.0
    ry, rx, oy, ox = gr.residual(cc)  # a peak at (0, 0): the samples at row 7 / column 9 are its neighbours
    assert oy == pytest.approx(0.5 * (1 - 2) / (1 - 8 + 2)) and ry == oy
    assert ox == 0.0 and rx == 0.0  # equal outer samples across the wrap
    cc = np.zeros((8, 10))
    cc[6, 7] = 1.0
    assert gr.residual(cc) == (-2.0, -3.0, 0.0, 0.0)  # wrap-around rule: p if p <= n // 2 else p - n
    cc = np.zeros((8, 10))
    cc[4, 5] = 1.0
    assert gr.residual(cc)[:2] == (4.0, 5.0)
    cc[2, 2] = 1.0  # a tie: the first maximum
    assert gr.residual(cc)[:2] == (2.0, 2.0)


@pytest.mark.parametrize("ref", [None, 0, -1, 5])
def test_reference_row_is_exactly_zero(planted, ref):
    S, shape, _ = planted
    s, _, _ = gr.refine_shifts(S, shape, reference_frame=ref, max_iterations=2, threshold=0.0)
    r = len(S) // 2 if ref is None else ref % len(S)
    assert s[r, 0] == 0.0 and s[r, 1] == 0.0
    assert np.abs(s).max() > 1.0


def test_one_frame_gives_zeros_and_bad_reference_raises():
    one = torch.randn(1, 64, 64)
    field, hist = gr.refine_global_motion(one, 1.0, return_history=True)
    assert tuple(field.shape) == (2, 1, 1, 1) and not field.any() and hist == []
    for bad in (8, -9):
        with pytest.raises(IndexError):
            gr.refine_global_motion(torch.randn(8, 64, 64), 1.0, reference_frame=bad)
        with pytest.raises(IndexError):
            gr.refine_shifts(np.zeros((8, 4, 3), dtype=complex), (4, 4), reference_frame=bad)


def test_restatement_field_layout():
    t, h, w = 3, 128, 128
    movie, _ = gr.planted_movie(t, h, w, [0.0, 0.3, 0.7], [0.0, -0.2, -0.4], noise=0.25, seed=2)
    field = gr.refine_global_motion(movie, 1.5, max_iterations=3, convergence_threshold=0.0)
    s, _, _ = gr.refine_shifts(gr.filtered_spectra(movie, 1.5), (h, w), max_iterations=3, threshold=0.0)
    assert field.dtype == torch.float64 and tuple(field.shape) == (2, t, 1, 1)
    assert np.array_equal(field[:, :, 0, 0].numpy().T, s * 1.5)
    # a caller's start field equal to the converged one stays there
    again = gr.refine_global_motion(movie, 1.5, deformation_field=field, max_iterations=1, convergence_threshold=0.0)
    assert float((again - field).abs().max()) < 0.01 * 1.5


# ------------------------------------------------------------------ argument rules of the public functions


def test_refine_global_motion_is_exported():
    assert callable(mc.refine_global_motion) and "refine_global_motion" in mc.__all__
    assert callable(mc.refine_global_motion_raw) and "refine_global_motion_raw" in mc.__all__
    assert callable(engine.refine_shifts_from_spectra) and callable(engine.global_shifts_refined)
    assert callable(engine.global_shifts_raw_refined)


def _refuse_devices(monkeypatch):
    from torch_motion_correction_amd import api

    def refuse(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    monkeypatch.setattr(api, "require_gpu", refuse)
    monkeypatch.setattr(api, "device_scope", refuse)


def test_refine_global_motion_argument_rules(monkeypatch):
    _refuse_devices(monkeypatch)
    img = torch.zeros(4, 64, 64)
    with pytest.raises(ValueError, match="image must be"):
        mc.refine_global_motion(torch.zeros(64, 64), 1.0)
    for bad in (0, -1, 2.5, True, None, "3"):
        with pytest.raises(ValueError, match="max_iterations"):
            mc.refine_global_motion(img, 1.0, max_iterations=bad)
    for bad in (-0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="convergence_threshold"):
            mc.refine_global_motion(img, 1.0, convergence_threshold=bad)
    for bad in (4, -5):
        with pytest.raises(IndexError):
            mc.refine_global_motion(img, 1.0, reference_frame=bad)
    with pytest.raises(ValueError, match="single patch"):
        mc.refine_global_motion(img, 1.0, deformation_field=torch.zeros(2, 4, 2, 2))
    with pytest.raises(ValueError, match="time points"):
        mc.refine_global_motion(img, 1.0, deformation_field=torch.zeros(2, 3, 1, 1))
    with pytest.raises(ValueError, match="deformation_grid must be"):
        mc.refine_global_motion(img, 1.0, deformation_field=torch.zeros(4, 2))
    with pytest.raises(NotImplementedError, match="512"):
        mc.refine_global_motion(torch.zeros(513, 8, 8), 1.0)


def test_refine_global_motion_raw_argument_rules(monkeypatch):
    _refuse_devices(monkeypatch)
    raw = torch.zeros(3, 512, 512, dtype=torch.uint8)
    with pytest.raises(ValueError, match="movie must be"):
        mc.refine_global_motion_raw(raw[0], None, 1.0)
    with pytest.raises(ValueError, match="gain reference"):
        mc.refine_global_motion_raw(raw, torch.ones(4, 4), 1.0)
    with pytest.raises(ValueError, match="hot_pixel_threshold"):
        mc.refine_global_motion_raw(raw, None, 1.0, hot_pixel_threshold=0.0)
    for bad in (0, 1.5, True, None):
        with pytest.raises(ValueError, match="max_iterations"):
            mc.refine_global_motion_raw(raw, None, 1.0, max_iterations=bad)
    for bad in (-1.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="convergence_threshold"):
            mc.refine_global_motion_raw(raw, None, 1.0, convergence_threshold=bad)
    with pytest.raises(IndexError):
        mc.refine_global_motion_raw(raw, None, 1.0, reference_frame=3)
    with pytest.raises(ValueError, match="time points"):
        mc.refine_global_motion_raw(raw, None, 1.0, deformation_field=torch.zeros(2, 4, 1, 1))


def test_engine_refine_rules():
    assert engine.check_refine_args(3, 0) == (3, 0.0)
    assert engine.check_refine_args(np.int64(2), np.float32(0.5)) == (2, 0.5)
    assert engine.check_refine_args(0, 0.01, min_iterations=0) == (0, 0.01)
    # the under-correction lies inside the 64 rows per end the near-window search visits, and inside small maps
    assert engine.refine_under_px(1024, 1024) == 16 and engine.refine_under_px(4096, 4096) == 16
    assert engine.refine_under_px(96, 120) == 16 and engine.refine_under_px(32, 64) == 8
    for h, w in [(8, 8), (32, 64), (96, 120), (4096, 4096)]:
        assert 1 <= engine.refine_under_px(h, w) < min(h, w) // 2
