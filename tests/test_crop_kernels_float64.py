"""Fourier cropping against the float64 definitions of tests/crop_reference.py: the cropping column pass
(csrc/fourier_crop.hip, mc_full_cols_crop) ALONE against cols_crop64, bin by bin, and the routes -- fourier_crop,
fourier_crop_raw on u8 / i16 with a gain, with and without the frame mean, with a hot-pixel list, an fp16 stack, an
input that is not 16-byte aligned, several chunks, an input whose energy lies in the discarded band -- against crop64,
per frame, no pixel excluded.  Every buffer the engine takes from torch.empty is NaN-filled (nan_empty) and the column
pass writes into a NaN-filled, NaN-guarded buffer, so a bin that a workgroup skips fails its comparison instead of
showing a former result; every test asserts which entry points of libmcorr ran.

Bounds (crop_reference's docstring derives them; none is fitted to a kernel's output).  They are ABSOLUTE: the
forward passes err relative to the input's norm, the inverse relative to what the crop leaves,

  frame   ||got - crop64(x)||_2 <= (2 (c_fwd ||x|| + extra) + (c_inv + 2 u) ||ref||) / (1 - c_fwd - c_inv)
  column  ||got - cols_crop64(s)||_2 <= (scale sqrt(H H/2) c_H ||s|| + (c_H/2 + u) ||ref||) / (1 - c_H - c_H/2)
  cap     every pixel / complex bin within 10 times the rms form of the same bound

Measured worst error / bound per family, from one run on an MI355X (L2 / per element); the fp32 CPU oracle's own
error over the same bounds on the same inputs is in the last column (tests/test_crop_reference_host.py):

                                                  kernels          fp32 CPU oracle
  column pass, H = 512                            0.033 / 0.015    0.021 / 0.009
  column pass, H = 1024                           0.030 / 0.012    0.018 / 0.006
  column pass, H = 2048                           0.028 / 0.011    0.017 / 0.006
  column pass, H = 4096                           0.027 / 0.013    0.016 / 0.006
  column pass, H = 8184 (mixed radix)             0.004 / 0.002    0.004 / 0.002
  fourier_crop, W = 128                           0.012 / 0.006    0.010 / 0.004
  fourier_crop, W = 256                           0.011 / 0.005    0.009 / 0.004
  fourier_crop, W = 512                           0.010 / 0.005    0.009 / 0.004
  fourier_crop, W = 1024                          0.011 / 0.006    0.010 / 0.004
  fourier_crop, W = 2048                          0.010 / 0.005    0.008 / 0.004
  fourier_crop, W = 4096                          0.010 / 0.006    0.008 / 0.004
  fourier_crop, W = 8192                          0.010 / 0.005    0.008 / 0.004
  fourier_crop, W = 11520                         0.008 / 0.004    0.009 / 0.004
  fourier_crop, input 4 bytes past 16             0.012 / 0.005    0.010 / 0.004
  discarded band (the forward term alone)         0.010 / 0.005    0.009 / 0.004
  several chunks                                  0.011 / 0.005    0.010 / 0.004
  raw u8 / i16, gain, with / without the mean     0.016 / 0.014    0.010 / 0.006
  raw u8 with a hot-pixel list                    0.009 / 0.001    0.006 / 0.002
  fp16 stack                                      0.011 / 0.006    0.010 / 0.005

The kernels sit at or within a factor 1.7 of torch's fp32 transform on the CPU in every family; no figure is far
below the oracle's.  Both are small against 1 because the bound is a worst case over all inputs (Higham's eta per
level adds linearly, rounding errors add like noise), and smallest at 8184 rows, where radix_cost takes the radix-31,
-11 and -24 butterflies as direct sums; the hot-pixel terms are added by the triangle inequality.  What the bound must
do it does: tests/test_crop_reference_host.py plants eight defects in the float64 restatement and each exceeds it on
every table case.

What the run showed: fourier_crop of an fp32 stack that starts 4 bytes past a 16-byte boundary raised McorrUnsupported
-- mc_full_rows_forward reads pairs of samples and refuses a pointer that is not 8-byte aligned.  engine._rows_forward
now copies such a stack, a chunk of frames at a time, into an aligned buffer; no kernel was changed.

Every test of this file takes half a second or less."""

import numpy as np
import pytest
import torch

import crop_reference as cr
import kernel_harness as kh
from kernel_harness import calls, mc, nan_empty, switches  # noqa: F401

pytestmark = pytest.mark.gpu

ratios = kh.ratios_fixture()
FWD, FWD_RAW = "mc_full_rows_forward", "mc_full_rows_forward_raw"
CROP, INV, HOT_FIX = "mc_full_cols_crop", "mc_full_rows_inverse", "mc_full_rows_hot_correct"
CONDITION = ("mc_condition_movie", "mc_condition_movie_hot")


def _worse(ratios, family, l2, px):
    kh.worse(ratios, family + " [L2]", l2)
    kh.worse(ratios, family + " [element]", px)


# ------------------------------------------------------------------ the column pass alone


def _launch_cols(calls, S, H, W, pitch, pitch2, tw, dev):
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    S2, flat = kh.nan_buffer((cr.COLS_JOBS, H // 2, pitch2, 2), dev)
    check(calls.mc_full_cols_crop(ptr(S), ptr(S2), ptr(tw), cr.COLS_JOBS, H, W, pitch, pitch2, stream_ptr(dev)), CROP)
    torch.cuda.synchronize()
    kh.assert_guards(S2, flat, f"{CROP} {H}x{W}")
    return S2


@pytest.mark.parametrize("case", cr.COLS_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_column_pass_matches_float64_bin_by_bin(calls, dev, ratios, case):
    """mc_full_cols_crop called as engine.fourier_crop calls it, on 2 jobs of different complex N(0, 1) data.  Every
    column of S from W/4 + 2 on is NaN, spectrum and pitch padding alike (the pair-wide kernels read W/4 + 1 as the
    partner of W/4; nothing beyond it may be read).  Every bin of columns 0 .. W/4 of S2, all rows, both jobs, is
    finite and inside cols_bound, per column in L2 and per bin; nothing is written outside S2; a second launch gives
    the same bits (the forward and the inverse transform share one LDS line).  S2's padding columns W/4 + 1 ..
    pitch2 - 1 are unspecified and NOT asserted."""
    from torch_motion_correction_amd import plan

    H, W = case
    lib = calls._lib
    pitch, pitch2 = lib.mc_full_spectrum_pitch(W), lib.mc_full_spectrum_pitch(W // 2)
    nk = W // 4 + 1
    assert pitch >= W // 2 + 1 and pitch2 >= nk + 1
    data = cr.cols_input(H, W)
    S = kh.nan((cr.COLS_JOBS, H, pitch, 2), dev)
    S[:, :, : nk + 1] = torch.from_numpy(data).to(dev)
    assert bool(torch.isnan(S[:, :, nk + 1:]).all()) and bool(torch.isfinite(S[:, :, : nk + 1]).all())
    tw = plan.get_twiddles(H, dev)
    first = _launch_cols(calls, S, H, W, pitch, pitch2, tw, dev)
    second = _launch_cols(calls, S, H, W, pitch, pitch2, tw, dev)
    calls.only(CROP, 2)
    got = first[:, :, :nk].cpu()
    assert bool(torch.isfinite(got).all()), f"{CROP} {case}: a bin of columns 0 .. W/4 is not finite (or was not written)"
    assert torch.equal(got.view(torch.int32), second[:, :, :nk].cpu().view(torch.int32)), "two launches differ"
    l2, px, _ = cr.cols_ratios(got.numpy(), cr.cols_crop64(data, H, W), data, H, W)
    print(f"{CROP} {H}x{W}: L2 {l2:.3f} bin {px:.3f}")
    _worse(ratios, f"cols H={H}", l2, px)
    assert l2 <= 1 and px <= 1, (l2, px)


# ------------------------------------------------------------------ the routes


def _assert_frames(got, ref, x_norms, h, w, what, extra=None, fwd_more=0.0, hot=None, fwd_only=False):
    """Every frame finite, within frame_bound in L2 and at every pixel -> worst (L2, pixel) ratio."""
    got = got.detach().cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite (or unwritten) output"
    worst = [0.0, 0.0]
    for f in range(ref.shape[0]):
        b = cr.frame_bound(h, w, float(x_norms[f]), float(torch.linalg.norm(ref[f])),
                           0.0 if extra is None else float(extra[f]), fwd_more, 0.0 if hot is None else float(hot[f]))
        if fwd_only:
            b = dict(b, l2=b["fwd"], cap=b["cap"] * b["fwd"] / b["l2"])
        l2, px = cr.frame_ratios(got[f], ref[f], b)
        print(f"  {what} frame {f}: L2 {l2:.3f} pixel {px:.3f}")
        assert l2 <= 1 and px <= 1, f"{what} frame {f}: error / bound L2 {l2:.3f} pixel {px:.3f}"
        worst = [max(worst[0], l2), max(worst[1], px)]
    return worst


def _norms(x):
    return [float(torch.linalg.norm(f.double())) for f in x]


@pytest.mark.parametrize("case", cr.ROUTE_CASES, ids=cr.case_id)
def test_fourier_crop_matches_float64(mc, dev, calls, nan_empty, ratios, case):
    """fourier_crop on fp32 frames: mc_full_rows_forward -> mc_full_cols_crop -> mc_full_rows_inverse, every pixel
    of every frame.  The last case starts 1 float past a 16-byte boundary."""
    t, h, w, offset = case
    x, ref = cr.frames_reference(t, h, w)
    xd = kh.offset_copy(x.to(dev), offset) if offset else x.to(dev)
    assert xd.data_ptr() % 16 == 4 * offset
    got = mc.fourier_crop(xd)
    torch.cuda.synchronize()
    calls.ran(FWD, CROP, INV, absent=(FWD_RAW, HOT_FIX) + CONDITION)
    assert calls.count(CROP) == 1 and calls.args[CROP][0][3:6] == (t, h, w)
    assert torch.equal(xd.cpu(), x)  # the input is not modified
    _worse(ratios, f"routes W={w}" + (" offset" if offset else ""),
           *_assert_frames(got, ref, _norms(x), h, w, f"fourier_crop {case}"))


def test_discarded_band_input(mc, dev, calls, nan_empty, ratios):
    """Energy only where the crop discards it: the reference is the image of the input's own fp32 rounding
    (||ref|| <= 2 u ||x||, asserted on the host too), and the output lies within the forward term 2 c_fwd ||x|| of
    the bound ALONE -- thousands of times ||ref||, which no criterion relative to the output can express."""
    t, h, w = cr.DISCARDED
    x = cr.discarded_band(t, h, w, seed=h + w)
    ref = cr.crop64(x)
    for f in range(t):
        assert float(torch.linalg.norm(ref[f])) <= cr.A_CROP * cr.U * float(torch.linalg.norm(x[f].double()))
    got = mc.fourier_crop(x.to(dev))
    torch.cuda.synchronize()
    calls.ran(FWD, CROP, INV, absent=(FWD_RAW,))
    _worse(ratios, "discarded band", *_assert_frames(got, ref, _norms(x), h, w, "discarded band", fwd_only=True))


def test_several_chunks(mc, dev, calls, nan_empty, switches, ratios):
    """WORKSPACE_BYTES cut to two frames of S and S2: chunks of 2 + 2 + 1 frames, the inverse row pass writing at
    per-chunk offsets; the bits of the one-chunk result, every frame within the bound."""
    engine, _ = switches
    t, h, w = cr.CHUNKS
    x, ref = cr.frames_reference(t, h, w)
    xd = x.to(dev)
    whole = mc.fourier_crop(xd)
    torch.cuda.synchronize()
    assert calls.count(CROP) == 1 and calls.args[CROP][0][3] == t
    calls.clear()
    lib = calls._lib
    engine.WORKSPACE_BYTES = 2 * (h * lib.mc_full_spectrum_pitch(w) + (h // 2) * lib.mc_full_spectrum_pitch(w // 2)) * 8
    got = mc.fourier_crop(xd)
    torch.cuda.synchronize()
    assert calls.count(FWD) == 3 and calls.count(CROP) == 3 and calls.count(INV) == 3
    assert [a[3] for a in calls.args[CROP]] == [2, 2, 1]
    assert torch.equal(got.cpu().view(torch.int32), whole.cpu().view(torch.int32))
    _worse(ratios, "chunks", *_assert_frames(got, ref, _norms(x), h, w, f"chunks {cr.CHUNKS}"))


@pytest.mark.parametrize("dtype,mean_zero", cr.RAW_CASES, ids=[f"{d}-{'mean_zero' if m else 'as_is'}" for d, m in cr.RAW_CASES])
def test_fourier_crop_raw_matches_float64(mc, dev, calls, nan_empty, ratios, dtype, mean_zero):
    """fourier_crop_raw with a gain of large dynamic range: the reference conditions in float64 with the kernels' own
    fp32 frame means (engine.RawMovie.mu; zero without mean_zero) and the bound carries the conditioning roundings in
    L2 through the factor 2.  No fp32 movie: the raw row pass ran, no conditioning kernel and no fp32 row pass did."""
    from torch_motion_correction_amd import engine

    t, h, w = cr.RAW_SHAPE
    raw, gain = cr.raw_case(dtype)
    mu = engine.RawMovie(raw.to(dev), gain.to(dev), mean_zero=mean_zero).mu.cpu().numpy()
    assert mean_zero or not mu.any()
    v, ref, cond = cr.raw_reference(raw.numpy(), gain.numpy(), mu)
    calls.clear()
    got = mc.fourier_crop_raw(raw.to(dev), gain.to(dev), mean_zero=mean_zero)
    torch.cuda.synchronize()
    calls.ran(FWD_RAW, CROP, INV, absent=(FWD, HOT_FIX) + CONDITION)
    x_norms = [np.linalg.norm(v[f]) for f in range(t)]
    _worse(ratios, "raw", *_assert_frames(got, ref, x_norms, h, w, f"fourier_crop_raw {dtype} mean_zero={mean_zero}",
                                          extra=cond))


def test_fourier_crop_raw_with_hot_pixels_matches_float64(mc, dev, calls, nan_empty, ratios):
    """The hot-pixel list enters the spectra as sparse corrections (mc_full_rows_hot_correct): against crop64 of the
    float64 rule's replaced movie (hot_reference.hot64; no pixel of the input is undecided) minus the kernels' fp32
    means after replacement, with the `hot` terms of crop_reference's bound.  The counts equal the reference's."""
    from torch_motion_correction_amd import engine

    raw, gain, ref64, x = cr.hot_case()
    t, h, w = x.shape
    thr = cr.RAW_HOT[1]
    rd, gd = torch.from_numpy(raw).to(dev), torch.from_numpy(gain).to(dev)
    mu = engine.RawMovie(rd, gd, hot_pixel_threshold=thr).mu.cpu().numpy()
    want, c_norm, extra, hot, more = cr.hot_reference_frames(raw, gain, ref64, x, mu)
    calls.clear()
    got, counts = mc.fourier_crop_raw(rd, gd, hot_pixel_threshold=thr, return_hot_counts=True)
    torch.cuda.synchronize()
    calls.ran(FWD_RAW, HOT_FIX, CROP, INV, absent=(FWD,) + CONDITION)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), ref64.counts)
    _worse(ratios, "raw hot", *_assert_frames(got, want, c_norm, h, w, "fourier_crop_raw hot pixels", extra=extra,
                                              fwd_more=more, hot=hot))


def test_fp16_stack_gives_the_bits_of_the_upcast_input(mc, dev, calls, nan_empty, ratios):
    t, h, w = cr.FP16
    half = cr.case_frames(t, h, w).half()
    got = mc.fourier_crop(half.to(dev))
    torch.cuda.synchronize()
    calls.ran(FWD, CROP, INV, absent=(FWD_RAW,))
    calls.clear()
    wide = mc.fourier_crop(half.float().to(dev))
    torch.cuda.synchronize()
    calls.ran(FWD, CROP, INV)
    assert got.dtype == torch.float32 and torch.equal(got.cpu().view(torch.int32), wide.cpu().view(torch.int32))
    x = half.float()
    _worse(ratios, "fp16", *_assert_frames(got, cr.crop64(x), _norms(x), h, w, f"fp16 {cr.FP16}"))
