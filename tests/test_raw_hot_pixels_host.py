"""Host-side checks of the fused raw path's hot-pixel step: argument validation of the new C entry points
and of the Python layer (no GPU touched), and the identity the K1 correction kernel implements."""

import ctypes
import math

import numpy as np
import pytest
import torch

from torch_motion_correction_amd import _lib, engine, plan

BAD_THRESHOLDS = [0.0, -1.0, float("nan"), float("inf"), float("-inf")]


def test_hot_entry_points_reject_bad_arguments_without_touching_the_gpu():
    lib = _lib.load()
    fake = lambda a: ctypes.c_void_p(a)  # noqa: E731
    p = [fake(0x10000 * (i + 1)) for i in range(10)]
    U8 = 0

    def detect(raw=p[0], gain=p[1], t=4, h=64, w=64, box=(16, 48, 16, 48), thr=10.0, cap=100, counter=p[6]):
        return lib.mc_raw_hot_detect(raw, U8, gain, t, h, w, *box, thr, p[2], p[3], p[4], p[5], cap, counter,
                                     p[7], None)

    assert detect(raw=None) == -1 and detect(gain=None) == -1 and detect(counter=None) == -1
    for thr in BAD_THRESHOLDS:
        assert detect(thr=thr) == -1, thr
    assert detect(t=0) == -1 and detect(cap=0) == -1 and detect(box=(16, 80, 16, 48)) == -1
    assert detect(w=60) == -2  # rows of whole 8-sample groups only: the caller falls back
    assert lib.mc_raw_hot_detect(p[0], 9, p[1], 4, 64, 64, 16, 48, 16, 48, 10.0, p[2], p[3], p[4], p[5], 100, p[6],
                                 p[7], None) == -2

    fin = lambda keys=p[0], n=5, t=4, stats=p[3]: lib.mc_raw_hot_finalize(  # noqa: E731
        keys, p[1], n, t, 64, 64, 16, 48, 16, 48, 1, p[2], stats, p[4], p[5], p[6], None)
    assert fin(keys=None) == -1 and fin(n=-1) == -1 and fin(t=0) == -1 and fin(stats=None) == -1

    g = plan.xc_geometry(512, 1024, 0.1, 16, 8)
    k1 = lambda keys=p[0], n=5, w=1024, T1=p[4], njobs=2: lib.mc_xc_rows_hot_correct(  # noqa: E731
        keys, p[1], n, 0, njobs, 512, w, p[2], p[3], T1, g, None)
    assert k1(keys=None) == -1 and k1(T1=None) == -1 and k1(n=-1) == -1 and k1(njobs=0) == -1
    assert k1(w=2048) == -1  # geometry of another width
    assert k1(n=0) == 0      # nothing to correct: no launch at all

    taps = lambda keys=p[0], scratch=p[2], n=5, h=64: lib.mc_warp_rigid_hot_taps(  # noqa: E731
        keys, p[1], n, 4, h, 64, scratch, p[3], p[4], None)
    assert taps(keys=None) == -1 and taps(scratch=None) == -1 and taps(n=-1) == -1 and taps(h=1) == -1
    assert taps(n=0) == 0
    add = lambda key=p[0], m=5, limit=100, out=p[2]: lib.mc_hot_scatter_add(key, p[1], m, limit, out, None)  # noqa: E731
    assert add(key=None) == -1 and add(out=None) == -1 and add(m=-1) == -1 and add(limit=0) == -1
    assert add(m=0) == 0


@pytest.mark.parametrize("thr", BAD_THRESHOLDS + ["ten"])
def test_python_layer_rejects_bad_thresholds_before_any_device(thr):
    import torch_motion_correction_amd as mc

    raw = torch.zeros((2, 64, 64), dtype=torch.uint8)  # CPU tensors: no device is ever needed
    with pytest.raises(ValueError, match="hot_pixel_threshold"):
        mc.motion_correct_raw(raw, None, 1.0, hot_pixel_threshold=thr)
    with pytest.raises(ValueError, match="hot_pixel_threshold"):
        mc.RawMoviePipeline(None, torch.device("cpu"), 1.0, hot_pixel_threshold=thr)
    with pytest.raises(ValueError, match="hot_pixel_threshold"):
        engine.RawMovie(raw, None, hot_pixel_threshold=thr)


def test_threshold_validation_accepts_finite_positive_values():
    assert engine.check_hot_pixel_threshold(None) is None
    assert engine.check_hot_pixel_threshold(10) == 10.0
    assert engine.check_hot_pixel_threshold(np.float32(0.5)) == 0.5
    assert engine.hot_list_capacity(40, 4096, 4096) == 40 * 4096
    assert engine.hot_list_capacity(2, 64, 64) == 4096


def test_k1_correction_identity_sign_scale_and_bins():
    """What mc_xc_rows_hot_correct adds: K1 transforms A = (v - sub) * rstd * mask along each row with the
    forward rfft (no scale, exp(-2 pi i kx x / W)) and keeps the first nkx bins.  Replacing v by r at a few
    pixels changes the kept bins of those rows by the sum of dA * exp(-2 pi i kx x / W) terms, dA = (r - v) *
    rstd * mask(y, x); pixels where the mask is zero and rows without hot pixels contribute nothing."""
    rng = np.random.default_rng(3)
    H, W, nkx = 24, 64, 21
    yy, xx = np.mgrid[0:H, 0:W]
    mask = np.clip(1.0 - np.hypot(yy - H // 2, xx - W // 2) / 14.0, 0.0, 1.0)  # zero outside a disk
    v = rng.normal(30.0, 5.0, (H, W))
    sub, rstd = 29.0, 1.0 / 5.0
    hot = [(12, 32, 400.0), (12, 33, 380.0), (5, 30, -200.0), (0, 0, 500.0), (20, 40, 300.0)]  # (0, 0): mask 0
    r = v.copy()
    for y, x, val in hot:
        r[y, x] = val
    A = (v - sub) * rstd * mask
    Ar = (r - sub) * rstd * mask
    T1 = np.fft.rfft(A, axis=1)[:, :nkx]
    T1r = np.fft.rfft(Ar, axis=1)[:, :nkx]
    corr = np.zeros_like(T1)
    kx = np.arange(nkx)
    for y, x, val in hot:
        dA = (val - v[y, x]) * rstd * mask[y, x]
        ph = (kx * x) % W  # the kernel's exact integer phase index
        corr[y] += dA * np.exp(-2j * np.pi * ph / W)
    np.testing.assert_allclose(T1 + corr, T1r, rtol=0, atol=1e-9 * np.abs(T1r).max())
    assert np.all(corr[0] == 0) and np.abs(corr[12]).max() > 0
    # torch's rfft (the convention K1 mirrors) agrees
    tr = torch.fft.rfft(torch.from_numpy(Ar), dim=1)[:, :nkx].numpy()
    np.testing.assert_allclose(tr, T1r, rtol=0, atol=1e-9 * np.abs(T1r).max())
    assert math.isclose(float(np.abs(corr[5, 0])), abs((-200.0 - v[5, 30]) * rstd * mask[5, 30]))
