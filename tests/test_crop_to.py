"""Fourier cropping to a given size on the GPU: fourier_crop_to and fourier_crop_to_raw against the float64 definition
(tests/crop_to_reference.py: crop_to64, which tests/test_crop_to_host.py pins) and against the compositions they are
defined as; the cropping column pass (csrc/fourier_crop_to.hip, mc_full_cols_crop_to) alone against its float64
restatement.  Every buffer the engine takes from torch.empty is NaN-filled (nan_empty) and the column pass writes into
a NaN-filled, NaN-guarded buffer, so a bin that a workgroup skips fails its comparison; every test asserts which entry
points of libmcorr ran.

The bounds are crop_to_reference's (derived there; none is fitted to a kernel's output), absolute and relative to the
INPUT's norm:  ||got - crop_to64(x)||_2 <= (A (c_fwd ||x|| + extra) + (c_inv + 2 u) ||ref||) / (1 - c_fwd - c_inv),
A = sqrt(H W / (H2 W2)), and every pixel within 10 times its rms form.  Each test prints its error over the bound and
its range_err (max |a - b| / range of b, as tests/test_fourier_crop.py prints it).

Every case takes a few seconds at most; the whole-frame case spends them in the float64 transform on the CPU."""

import numpy as np
import pytest
import torch

import crop_reference as cr
import crop_to_reference as ct
import kernel_harness as kh
from kernel_harness import calls, mc, nan_empty, switches  # noqa: F401

pytestmark = pytest.mark.gpu

FWD, FWD_RAW = "mc_full_rows_forward", "mc_full_rows_forward_raw"
CROP_TO, CROP, INV, HOT_FIX = "mc_full_cols_crop_to", "mc_full_cols_crop", "mc_full_rows_inverse", "mc_full_rows_hot_correct"
CONDITION = ("mc_condition_movie", "mc_condition_movie_hot")


def range_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.max() - b.min()), 1e-30))


def _norms(x):
    return [float(torch.linalg.norm(f.double())) for f in x]


def _assert_frames(got, ref, x_norms, shape, out_shape, what, bound=None):
    """Every frame finite, within frame_bound in L2 and at every pixel.  `bound(f, b)`: the frame's bound from the
    plain one."""
    _, h, w = shape
    got = got.detach().cpu()
    assert got.shape == ref.shape and got.dtype == torch.float32, (got.shape, ref.shape, got.dtype)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite (or unwritten) output"
    for f in range(ref.shape[0]):
        b = ct.frame_bound(h, w, *out_shape, float(x_norms[f]), float(torch.linalg.norm(ref[f])))
        if bound is not None:
            b = bound(f, b)
        l2, px = ct.frame_ratios(got[f], ref[f], b)
        print(f"  {what} frame {f}: error / bound L2 {l2:.3f} pixel {px:.3f}, range_err {range_err(got[f], ref[f]):.3e}")
        assert l2 <= 1 and px <= 1, f"{what} frame {f}: error / bound L2 {l2:.3f} pixel {px:.3f}"


# ------------------------------------------------------------------ the column pass alone


COLS_JOBS = 2
COLS_CASES = [(512, 384, 256, 128), (4096, 3072, 128, 64), (4092, 2046, 128, 64), (8184, 5456, 128, 64),
              (8184, 2728, 128, 64), (512, 384, 1024, 512), (8184, 5456, 1024, 512)]  # the last two: XCD remap, tails


@pytest.mark.parametrize("case", COLS_CASES, ids=lambda c: "{}to{}-{}to{}".format(*c))
def test_column_pass_matches_float64_bin_by_bin(calls, dev, case):
    """mc_full_cols_crop_to called as the engine calls it, on 2 jobs of different complex N(0, 1) data.  Every column
    of S from W2/2 + 2 on is NaN, spectrum and pitch padding alike (the pair-wide kernels read W2/2 + 1 as the
    partner of W2/2; nothing beyond it may be read).  Every bin of columns 0 .. W2/2 of S2 is finite and inside
    cols_bound, per column in L2 and per bin; nothing is written outside S2; a second launch gives the same bits
    (the forward and the inverse transform share one LDS line)."""
    from torch_motion_correction_amd import plan
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    H, H2, W, W2 = case
    lib = calls._lib
    pitch, pitch2 = lib.mc_full_spectrum_pitch(W), lib.mc_full_spectrum_pitch(W2)
    nk = W2 // 2 + 1
    assert pitch >= pitch2 >= nk + 1
    data = kh.rng(H, H2, W2, 17).standard_normal((COLS_JOBS, H, nk + 1, 2)).astype(np.float32)
    S = kh.nan((COLS_JOBS, H, pitch, 2), dev)
    S[:, :, : nk + 1] = torch.from_numpy(data).to(dev)
    tw, tw2 = plan.get_twiddles(H, dev), plan.get_twiddles(H2, dev)
    out = []
    for _ in range(2):
        S2, flat = kh.nan_buffer((COLS_JOBS, H2, pitch2, 2), dev)
        check(calls.mc_full_cols_crop_to(ptr(S), ptr(S2), ptr(tw), ptr(tw2), COLS_JOBS, H, W, H2, W2, pitch, pitch2,
                                         stream_ptr(dev)), CROP_TO)
        torch.cuda.synchronize()
        kh.assert_guards(S2, flat, f"{CROP_TO} {case}")
        out.append(S2[:, :, :nk].cpu())
    calls.only(CROP_TO, 2)
    got = out[0]
    assert bool(torch.isfinite(got).all()), f"{CROP_TO} {case}: a bin of columns 0 .. W2/2 is not finite (or unwritten)"
    assert torch.equal(got.view(torch.int32), out[1].view(torch.int32)), "two launches differ"
    ref = ct.cols_crop_to64(data, H, H2, W2)
    z = cr._as_complex(data)[:, :, :nk]
    d = np.abs(cr._as_complex(got.numpy()) - ref)
    l2, cap = ct.cols_bound(H, H2, W2, np.linalg.norm(z, axis=1), np.linalg.norm(ref, axis=1))
    r_l2, r_px = float((np.sqrt((d * d).sum(axis=1)) / l2).max()), float((d.max(axis=1) / cap).max())
    print(f"{CROP_TO} {case}: error / bound L2 {r_l2:.3f} bin {r_px:.3f}")
    assert r_l2 <= 1 and r_px <= 1, (r_l2, r_px)


# ------------------------------------------------------------------ the route on fp32 frames


@pytest.mark.parametrize("case", ct.ROUTE_CASES, ids=ct.case_id)
def test_fourier_crop_to_matches_float64(mc, dev, calls, nan_empty, case):
    """fourier_crop_to on fp32 frames: mc_full_rows_forward -> mc_full_cols_crop_to -> mc_full_rows_inverse, every
    pixel of every frame."""
    shape, out_shape = case
    t, h, w = shape
    x, ref = ct.frames_reference(shape, out_shape)
    xd = x.to(dev)
    got = mc.fourier_crop_to(xd, out_shape)
    torch.cuda.synchronize()
    calls.ran(FWD, CROP_TO, INV, absent=(CROP, FWD_RAW, HOT_FIX) + CONDITION)
    assert calls.count(CROP_TO) == 1 and calls.args[CROP_TO][0][4:9] == (t, h, w, *out_shape)
    assert got.device == xd.device and torch.equal(xd.cpu(), x)  # the input is not modified
    _assert_frames(got, ref, _norms(x), shape, out_shape, f"fourier_crop_to {ct.case_id(case)}")


def test_whole_k3_counting_mode_frame(mc, dev, calls, nan_empty):
    shape, out_shape = ct.WHOLE_FRAME
    x = cr.case_frames(*shape)
    got = mc.fourier_crop_to(x.to(dev), out_shape)
    torch.cuda.synchronize()
    calls.ran(FWD, CROP_TO, INV, absent=(CROP,))
    _assert_frames(got, ct.crop_to64(x, out_shape), _norms(x), shape, out_shape, f"fourier_crop_to {shape}")


def test_column_and_row_edges(mc, dev, calls, nan_empty):
    """One frame per edge of the kept band, its spectrum a single impulse (and the Hermitian twin): ky = h2/2 - 1 and
    ky = h - h2/2 (the new Nyquist row) are kept, ky = h2/2 and ky = h - h2/2 - 1 dropped; kx = w2/2 is kept with
    its real part only (the phase 0.7 gives it an imaginary part to lose), kx = w2/2 + 1 dropped.  Each against the
    float64 answer within the bound; a kept impulse comes back with the input's norm times sqrt(A^2 / 2 .. A^2), a
    dropped one as the image of the fp32 rounding of the input alone."""
    (h, w), (h2, w2) = ct.EDGES
    edges = ct.edge_impulses(h, w, h2, w2)
    x = torch.stack([ct.impulse_frame(h, w, ky, kx) for _, (ky, kx), _ in edges]).float()
    ref = ct.crop_to64(x, (h2, w2))
    a = ct.amplification(h, w, h2, w2)
    for f, (name, _, kept) in enumerate(edges):
        ratio = float(torch.linalg.norm(ref[f]) / torch.linalg.norm(x[f].double()))
        assert (0.4 * a <= ratio <= 1.01 * a) if kept else (ratio <= a * ct.U), (name, ratio)
    got = mc.fourier_crop_to(x.to(dev), (h2, w2))
    torch.cuda.synchronize()
    calls.ran(FWD, CROP_TO, INV)
    _assert_frames(got, ref, _norms(x), (len(edges), h, w), (h2, w2), "edges")
    for f, (name, _, kept) in enumerate(edges):  # in plain words: a kept wave has amplitude A^2 (half at kx = w2/2)
        size = float(got[f].abs().max())
        assert (size > 0.45 * a * a) if kept else (size < 0.01 * a * a), (name, size)


def test_one_column_pass_per_chunk_and_the_same_bits(mc, dev, calls, nan_empty, switches):
    """WORKSPACE_BYTES cut to two frames of S and S2: two chunks of 2 frames, the inverse row pass writing at
    per-chunk offsets; the bits of the one-chunk result."""
    engine, _ = switches
    shape, out_shape = ct.CHUNKS
    t, h, w = shape
    x, ref = ct.frames_reference(shape, out_shape)
    xd = x.to(dev)
    whole = mc.fourier_crop_to(xd, out_shape)
    torch.cuda.synchronize()
    assert calls.count(CROP_TO) == 1 and calls.args[CROP_TO][0][4] == t
    calls.clear()
    lib = calls._lib
    engine.WORKSPACE_BYTES = 2 * (h * lib.mc_full_spectrum_pitch(w) + out_shape[0] * lib.mc_full_spectrum_pitch(out_shape[1])) * 8
    got = mc.fourier_crop_to(xd, out_shape)
    torch.cuda.synchronize()
    assert calls.count(FWD) == 2 and calls.count(CROP_TO) == 2 and calls.count(INV) == 2
    assert [a[4] for a in calls.args[CROP_TO]] == [2, 2]
    assert torch.equal(got.cpu().view(torch.int32), whole.cpu().view(torch.int32))
    _assert_frames(got, ref, _norms(x), shape, out_shape, f"chunks {shape}")


def test_the_halving_is_fourier_crop(mc, dev, calls, nan_empty):
    t, h, w = ct.HALVING
    xd = cr.case_frames(t, h, w).to(dev)
    want = mc.fourier_crop(xd)
    torch.cuda.synchronize()
    calls.clear()
    got = mc.fourier_crop_to(xd, (h // 2, w // 2))
    torch.cuda.synchronize()
    calls.ran(FWD, CROP, INV, absent=(CROP_TO,))
    assert got.shape == (t, h // 2, w // 2) and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_a_single_image_the_device_rule_and_fp16(mc, dev, calls, nan_empty):
    shape, out_shape = ct.ROUTE_CASES[0]
    x = cr.case_frames(*shape)
    stack = mc.fourier_crop_to(x.to(dev), out_shape)
    y = mc.fourier_crop_to(x[0].to(dev), out_shape)
    assert y.shape == out_shape and y.dtype == torch.float32 and y.device.type == "cuda" and torch.equal(y, stack[0])
    y_cpu = mc.fourier_crop_to(x[0], out_shape)  # a CPU image comes back on the CPU, computed on the GPU
    assert y_cpu.device.type == "cpu" and torch.equal(y_cpu, y.cpu())
    assert mc.fourier_crop_to(x[0], out_shape, device=dev).device.type == "cuda"
    calls.clear()
    y16 = mc.fourier_crop_to(x.half().to(dev), out_shape)  # fp16 is widened, the result is fp32
    calls.ran(FWD, CROP_TO, INV)
    assert y16.dtype == torch.float32
    assert torch.equal(y16.view(torch.int32), mc.fourier_crop_to(x.half().float().to(dev), out_shape).view(torch.int32))


# ------------------------------------------------------------------ the raw route


@pytest.mark.parametrize("dtype,with_gain,mean_zero", ct.RAW_CASES,
                         ids=[f"{d}-{'gain' if g else 'no_gain'}-{'mean_zero' if m else 'as_is'}" for d, g, m in ct.RAW_CASES])
def test_raw_without_hot_pixels_is_the_composition_bit_for_bit(mc, dev, calls, nan_empty, dtype, with_gain, mean_zero):
    shape, out_shape = ct.RAW
    t, h, w = shape
    dt = getattr(torch, dtype)
    raw = kh.raw_movie(t, h, w, dt, seed=900 + h + (1 if dt == torch.int16 else 0)).to(dev)
    gain = kh.gain(h, w).to(dev) if with_gain else None
    want = mc.fourier_crop_to(mc.condition_movie(raw, gain, mean_zero=mean_zero), out_shape)
    torch.cuda.synchronize()
    calls.clear()
    got = mc.fourier_crop_to_raw(raw, gain, out_shape, mean_zero=mean_zero)
    torch.cuda.synchronize()
    calls.ran(FWD_RAW, CROP_TO, INV, absent=(FWD, CROP, HOT_FIX) + CONDITION)  # no fp32 movie
    assert got.dtype == torch.float32 and got.shape == (t, *out_shape)
    assert bool(torch.isfinite(got).all()) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    got2, counts = mc.fourier_crop_to_raw(raw, gain, out_shape, mean_zero=mean_zero, return_hot_counts=True)
    assert torch.equal(got2, want) and counts.dtype == torch.int32 and counts.shape == (t,) and not counts.any()


def test_raw_with_hot_pixels_is_the_composition(mc, dev, calls, nan_empty):
    """With a threshold the fused route transforms the UNREPLACED samples c and adds, per list entry, dA = r - v to
    the spectra; the composition replaces first.  Both use the same fp32 samples, means and replacements r, so they
    are two fp32 evaluations of one exact value, the crop of (c with r at the list's pixels): the composition within
    the plain bound of it, the fused route within the bound with crop_to_reference's `hot` terms at e_r = 0 (the
    replacement's own error is common to both).  Their difference lies within the sum of the two.  The counts are
    equal, and the fused route conditions nothing."""
    import hot_reference as hr
    from torch_motion_correction_amd import engine

    shape, out_shape = ct.RAW
    t, h, w = shape
    kind, thr = ct.RAW_HOT
    raw, gain, _ = hr.hot_movie(kind, shape)
    rd, gd = torch.from_numpy(raw).to(dev), torch.from_numpy(gain).to(dev)
    img, want_counts = mc.condition_movie(rd, gd, hot_pixel_threshold=thr, return_hot_counts=True)
    want = mc.fourier_crop_to(img, out_shape)
    rm = engine.RawMovie(rd, gd, hot_pixel_threshold=thr)
    torch.cuda.synchronize()
    assert int(want_counts.sum()) > 0 and rm.n_hot == int(want_counts.sum())
    keys, rv = rm.hot_keys.cpu().numpy(), rm.hot_rv.cpu().double().numpy()
    rows, n_in_row = np.unique(keys // w, return_counts=True)
    n_row = n_in_row[np.searchsorted(rows, keys // w)]
    x_norms = _norms(img.cpu())
    calls.clear()
    got, counts = mc.fourier_crop_to_raw(rd, gd, out_shape, hot_pixel_threshold=thr, return_hot_counts=True)
    torch.cuda.synchronize()
    calls.ran(FWD_RAW, HOT_FIX, CROP_TO, INV, absent=(FWD, CROP) + CONDITION)
    assert torch.equal(counts, want_counts)

    def bound(f, plain):
        m = keys // (h * w) == f
        dA = rv[m, 0] - rv[m, 1]
        hot, more = cr.hot_terms(np.zeros(int(m.sum())), dA, n_row[m], w)
        # the unreplaced samples' norm: the replaced frame's, plus what the entries carry
        c_norm = x_norms[f] + float(np.linalg.norm(dA))
        fused = ct.frame_bound(h, w, *out_shape, c_norm, float(torch.linalg.norm(want[f])), fwd_more=more, hot=hot)
        return ct.added(plain, fused)

    _assert_frames(got, want.cpu().double(), x_norms, shape, out_shape, "fourier_crop_to_raw hot pixels", bound=bound)
    print(f"fourier_crop_to_raw hot pixels: range_err {range_err(got, want):.3e}")


# ------------------------------------------------------------------ what is refused


@pytest.mark.parametrize("case", ct.UNSUPPORTED, ids=ct.case_id)
def test_unsupported_pairs_raise_before_any_launch(mc, dev, case, monkeypatch):
    from torch_motion_correction_amd import engine

    def refuse(*a, **k):
        raise AssertionError("a kernel was about to be launched")

    monkeypatch.setattr(engine, "_rows_forward", refuse)
    monkeypatch.setattr(engine, "_raw_rows_forward", refuse)
    monkeypatch.setattr(engine.RawMovie, "__init__", refuse)
    monkeypatch.setattr(engine, "condition_movie", refuse)
    shape, out_shape = case
    raw = torch.zeros(shape, dtype=torch.uint8, device=dev)
    with pytest.raises(NotImplementedError, match="8184 -> 5456.*7680"):
        mc.fourier_crop_to(raw.float(), out_shape)
    with pytest.raises(NotImplementedError, match="8184 -> 5456.*7680"):
        mc.fourier_crop_to_raw(raw, None, out_shape)
    with pytest.raises(engine._lib.McorrUnsupported, match="8184 -> 5456.*7680"):
        engine.fourier_crop_to(raw.float(), out_shape)
