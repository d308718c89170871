"""Shared pieces of the Fourier-crop tests (tests/test_crop_reference_host.py, tests/test_crop_kernels_float64.py and,
through tests/test_fourier_crop_host.py, tests/test_fourier_crop.py): the definition in float64 (crop64), the column
pass csrc/fourier_crop.hip restated in float64 (cols_crop64), the error bounds derived from the arithmetic, and the
case tables the host and the GPU tests both run.  Everything here is float64 on the CPU and knows nothing of the
package's kernels; nothing is measured on a kernel.

The bounds.  Notation of tests/fourier_reference.py: u = 2^-24, eta = one radix-2 level with fp32-rounded twiddles
(Higham, Theorem 24.2), _fft_cost(n) the relative L2 error of one complex n-point line as the kernels factor it
(log2 n eta for a power of two, the pass list of smooth_radix_list otherwise).  Every pass is unitary up to a scale, so
to first order the relative errors of consecutive passes add; the factor 1 / (1 - c) below takes the higher orders.

The crop is NOT a round trip: the forward passes err relative to the norm of what they transform (the whole frame),
the crop is a projection that throws three quarters of a white spectrum away, and the inverse passes err relative to
what is left.  A bound relative to the output alone would therefore be wrong by the ratio of the two norms -- unbounded
for a frame whose energy sits in the discarded band.  The bound is absolute, with one term per side:

  frame   F = DFT2(x) unnormalised, ||F|| = sqrt(H W) ||x|| over the full (Hermitian) spectrum.  The fp32 row pass
          (a packed W/2-point line and the unpack level) and the H-point column pass give F + E,
              ||E|| <= c_fwd sqrt(H W) ||x||,     c_fwd = _fft_cost(W/2) + eta + _fft_cost(H).
          Cropping keeps bins (each kept bin once; the new Nyquist row and column are kept once where the input
          counted them twice) and the real inverse drops the imaginary parts of its DC and Nyquist bins: both are
          projections, of norm <= 1.  The unnormalised inverse at (H2, W2) = (H/2, W/2) multiplies norms by
          sqrt(H2 W2), and the scale is 1 / (H2 W2).  So E reaches the output as at most
              sqrt(H2 W2) / (H2 W2) * c_fwd sqrt(H W) ||x|| = sqrt(H W / (H2 W2)) c_fwd ||x|| = A c_fwd ||x||, A = 2.
          The inverse passes hold the cropped spectrum, whose image is the reference y = crop64(x):
              c_inv ||y||,     c_inv = _fft_cost(H/2) + _fft_cost(W/4) + eta (the pack level).
          The scale: the constant 1 / (H2 W2) rounded to fp32 (exact for powers of two, inexact at 8184 and 11520;
          crop64 divides by the exact product, so this rounding is a term, u ||y||) and the product with it
          (u ||y||): SCALE_FRAME = 2 u.  Stores round nothing (the values are fp32 already).
              frame_bound = (A (c_fwd ||x|| + extra) + (c_inv + 2 u) ||y||) / (1 - c_fwd - c_inv)
          `extra`: an absolute L2 error of the INPUT (the conditioning roundings of a raw movie, the hot-pixel
          corrections); it passes through the same A.

  column  the column pass alone, one column s (H complex samples) -> r = cols_crop64 (H2 samples).  Forward error
          c_H sqrt(H) ||s|| in the unnormalised spectrum, projection, unnormalised inverse sqrt(H2), scale:
              a_col = scale sqrt(H H2),   cols_bound = (a_col c_H ||s|| + (c_H2 + u) ||r||) / (1 - c_H - c_H2)
          with c_H = _fft_cost(H), c_H2 = _fft_cost(H/2).  cols_crop64 multiplies by the SAME fp32-rounded scale as
          the kernel (it is an argument of the pass), so only the product's rounding u remains.

  cap     per element (a pixel of a frame, a complex bin of a column by its modulus): CAP = 10 times the rms form of
          the same bound, bound / sqrt(number of elements) -- the project's rule (fourier_reference.bounds).  It rests
          on the fp32 CPU oracle's own error being noise-like, max / rms <= MAX_OVER_RMS = 8 on every table case,
          which tests/test_crop_reference_host.py asserts.

  hot     a raw movie with a hot-pixel list: the kernels transform the UNREPLACED conditioned samples c and add, per
          list entry, dA = r - v times exp(-2 pi i kx x / W) to the W/2 + 1 bins of the entry's row
          (mc_full_rows_hot_correct).  Against crop64 of the replaced movie: ||c|| of the transformed (unreplaced)
          samples takes ||x||'s place and its conditioning roundings go into `extra`; the addition onto the
          spectrum rounds once more relative to the bin (u more in c_fwd); each entry adds the fp32 replacement's
          own error e_r (hot_reference.replacement_error64) at its pixel, L2 over the entries, and the error of its
          correction, per bin and component eps |dA| with eps = sqrt2 1e-6 + 2 pi u + 3 u + (n_row + 1) u
          (hot_reference's `rows` paragraph), i.e. a complex error of modulus <= sqrt2 eps |dA| on W/2 + 1 bins.  By
          Parseval for the W-point real row that is an input perturbation of norm <= sqrt((2 / W) (W/2 + 1))
          sqrt2 eps |dA| <= 2 eps |dA|; the entries' perturbations are added by the triangle inequality.
          These errors are NOT noise-like -- they sit at the entry's pixel and along its row -- so the per-pixel cap
          takes them by their maximum instead of CAP times their rms share: a perturbation d at one input pixel
          reaches an output pixel through the crop's point response, (1 / (H2 W2)) times a sum of at most
          H2 (W2 + 1) unit phasors, modulus <= 1 + 2 / W; a perturbation p along one row keeps that factor along y
          and along x passes the 1-D crop, whose L2 gain is sqrt(W / W2) = sqrt2, so max |.| <= sqrt2 ||p||_2.
              local = (1 + 2 / W) sqrt2 sum_entries (e_r + 2 eps |dA|),   cap = CAP (l2 - A hot) / sqrt(H2 W2) + local
"""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

import fourier_reference as fr
from fourier_reference import CAP, ETA, MAX_OVER_RMS, U, _fft_cost  # noqa: F401

F32 = np.float32
A_CROP = 2.0           # sqrt(H W / (H2 W2)), derived above
SCALE_FRAME = 2 * U    # the scale constant's rounding to fp32 and the product with it
SCALE_COLS = U         # the product alone: cols_crop64 shares the rounded constant


# ------------------------------------------------------------------ the definition


def crop64(x):
    """The definition, in float64 on the CPU: rows -h/4 <= ky < h/4 (signed; the new Nyquist row from the negative
    side) and columns 0 <= kx <= w/4 of rfft2(x), inverted at (h/2, w/2); irfft2's 1 / ((h/2)(w/2)) is the only
    scale.  One frame at a time (an 8184 x 11520 spectrum is 754 MB in complex128)."""
    x = x.detach().cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    if x.dim() == 3:
        return torch.stack([crop64(f) for f in x])
    x = x.double()
    h, w = x.shape
    h2, w2 = h // 2, w // 2
    F = torch.fft.rfft2(x)
    G = torch.cat((F[: h2 // 2, : w2 // 2 + 1], F[h - h2 // 2:, : w2 // 2 + 1]), dim=0)
    return torch.fft.irfft2(G, s=(h2, w2))


def band_limited(h, w, seed, t=None):
    """float64 frames whose spectrum is zero at and beyond the Nyquist frequencies of the (h/2, w/2) grid."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((h, w) if t is None else (t, h, w), generator=g, dtype=torch.float64)
    F = torch.fft.rfft2(x)
    F[..., h // 4: h - h // 4 + 1, :] = 0  # |ky| >= h/4
    F[..., :, w // 4:] = 0  # kx >= w/4
    return torch.fft.irfft2(F, s=(h, w))


def discarded_band(t, h, w, seed):
    """fp32 frames with energy only in the band the crop discards, |ky| > h/4 or kx > w/4: white noise with the kept
    band (and its rim) removed in float64, then rounded to fp32 -- so crop64 of them is that rounding's image only."""
    g = torch.Generator().manual_seed(seed)
    F = torch.fft.rfft2(torch.randn(t, h, w, generator=g, dtype=torch.float64))
    keep_rows = torch.cat((torch.arange(0, h // 4 + 1), torch.arange(h - h // 4, h)))
    F[:, keep_rows[:, None], torch.arange(0, w // 4 + 1)[None, :]] = 0
    return torch.fft.irfft2(F, s=(h, w)).float()


# ------------------------------------------------------------------ the column pass


def crop_scale(H, W):
    """The scale mc_full_cols_crop applies: float32(1 / ((H/2)(W/2))), widened back."""
    return float(F32(1.0 / (float(H // 2) * float(W // 2))))


def _as_complex(S):
    S = S.detach().cpu().numpy() if isinstance(S, torch.Tensor) else np.asarray(S)
    if np.iscomplexobj(S):
        return S.astype(np.complex128)
    assert S.shape[-1] == 2, S.shape
    return S[..., 0].astype(np.float64) + 1j * S[..., 1].astype(np.float64)


def cropped_columns64(S, H, W):
    """The kept rows of the forward column transform, unscaled: S[job][y][kx] (complex, or fp32 pairs in a last axis
    of 2; at least W/4 + 1 columns, the rest is ignored) -> G[job][ky'][kx], kx <= W/4, complex128: per column the
    unnormalised H-point DFT (sign -), rows ky < H/4 and ky >= 3H/4 placed at ky mod H/2."""
    z = _as_complex(S)[:, :, : W // 4 + 1]
    assert z.ndim == 3 and z.shape[1] == H and z.shape[2] == W // 4 + 1, (z.shape, H, W)
    F = np.fft.fft(z, axis=1)
    return np.concatenate((F[:, : H // 4], F[:, H - H // 4:]), axis=1)


def columns_inverse64(G, H, W):
    """The unnormalised H/2-point DFT (sign +) along ky' and the scale."""
    return np.fft.ifft(G, axis=1) * (H // 2) * crop_scale(H, W)


def cols_crop64(S, H, W):
    """mc_full_cols_crop restated: for each job and each kx <= W/4, along y, the unnormalised H-point DFT (sign -),
    the rows ky < H/4 and ky >= 3H/4 at ky mod H/2 (the new Nyquist row H/4 is ky = 3H/4, the negative side), the
    unnormalised H/2-point DFT (sign +), times crop_scale(H, W).  -> complex128 (jobs, H/2, W/4 + 1)."""
    return columns_inverse64(cropped_columns64(S, H, W), H, W)


def rows_inverse64(S2, W):
    """The float64 row transform that follows the column pass: S2 (jobs, H2, W/4 + 1) complex -> (jobs, H2, W/2) real,
    unnormalised (numpy's irfft times its length); the DC and Nyquist bins' imaginary parts are dropped."""
    return np.fft.irfft(S2, n=W // 2, axis=2) * (W // 2)


def rows_forward64(x):
    """(jobs, H, W) real -> (jobs, H, W/2 + 1) complex128, unnormalised, sign -."""
    return np.fft.rfft(np.asarray(x, dtype=np.float64), axis=2)


# ------------------------------------------------------------------ the bounds


def frame_costs(h, w):
    """(c_fwd, c_inv) of the module docstring."""
    return _fft_cost(w // 2) + ETA + _fft_cost(h), _fft_cost(h // 2) + _fft_cost(w // 4) + ETA


def frame_bound(h, w, x_norm, ref_norm, extra=0.0, fwd_more=0.0, hot=0.0):
    """Absolute L2 bound of one cropped frame against crop64: ||x||_2 of the (h, w) frame the forward passes
    transform, ||ref||_2 of its crop, `extra` an absolute L2 error of the input that is spread like noise,
    `fwd_more` further roundings relative to the forward spectrum, `hot` the sum over a hot-pixel list of the entries'
    localised input errors (the `hot` paragraph).  -> dict: fwd (the A c_fwd ||x|| term, higher orders included), l2,
    cap (per pixel)."""
    c_fwd, c_inv = frame_costs(h, w)
    c_fwd += fwd_more
    amp = 1.0 / (1.0 - c_fwd - c_inv)
    fwd = amp * A_CROP * c_fwd * x_norm
    spread = fwd + amp * (A_CROP * extra + (c_inv + SCALE_FRAME) * ref_norm)
    local = amp * (1.0 + 2.0 / w) * math.sqrt(2.0) * hot
    return {"fwd": fwd, "l2": spread + amp * A_CROP * hot,
            "cap": CAP * spread / math.sqrt((h // 2) * (w // 2)) + local}


def cols_bound(H, W, s_norm, r_norm):
    """Absolute L2 bound of one column (or an array of columns) of the column pass against cols_crop64: ||s||_2 of
    the H input samples, ||r||_2 of the H/2 reference samples.  -> (l2, cap per complex bin, by its modulus)."""
    c_h, c_h2 = _fft_cost(H), _fft_cost(H // 2)
    a_col = crop_scale(H, W) * math.sqrt(H * (H // 2))
    l2 = (a_col * c_h * np.asarray(s_norm) + (c_h2 + SCALE_COLS) * np.asarray(r_norm)) / (1.0 - c_h - c_h2)
    return l2, CAP * l2 / math.sqrt(H // 2)


def hot_terms(e_r, dA, n_row, W):
    """The `hot` paragraph: (`hot` of frame_bound, fwd_more) for list entries with replacement errors e_r,
    corrections dA = r - v and n_row entries in their row (in L2 the entries are added by the triangle inequality
    too, which is no smaller than the norm over distinct pixels)."""
    from hot_reference import TRIG

    eps = TRIG + 2 * math.pi * U + 3 * U + (np.asarray(n_row, dtype=np.float64) + 1) * U
    assert (2.0 / W) * (W // 2 + 1) * 2.0 <= 4.0
    return float((np.asarray(e_r) + 2.0 * eps * np.abs(dA)).sum()), U


# ------------------------------------------------------------------ comparisons (host oracle and kernels alike)


def frame_ratios(got, ref, bound):
    """(L2 error / bound, max |error| / cap) of one frame; a NaN gives inf."""
    d = fr._t64(got) - fr._t64(ref)
    if not bool(torch.isfinite(d).all()):
        return math.inf, math.inf
    return float(torch.linalg.norm(d)) / bound["l2"], float(d.abs().max()) / bound["cap"]


def cols_ratios(got, ref, S, H, W):
    """Worst (L2 error / bound, max |bin error| / cap) over every job and column kx <= W/4 of the column pass:
    `got`, `ref` complex (jobs, H/2, W/4 + 1), `S` the input.  A NaN gives inf.  Also -> max / rms of the error."""
    z = _as_complex(S)[:, :, : W // 4 + 1]
    d = np.abs(_as_complex(got) - ref)
    if not np.isfinite(d).all():
        return math.inf, math.inf, math.inf
    l2, cap = cols_bound(H, W, np.linalg.norm(z, axis=1), np.linalg.norm(ref, axis=1))
    err = np.sqrt((d * d).sum(axis=1))
    return float((err / l2).max()), float((d.max(axis=1) / cap).max()), float(d.max() / math.sqrt((d * d).mean()))


# ------------------------------------------------------------------ the cases

COLS_HEIGHTS = (512, 1024, 2048, 4096, 8184)
COLS_WIDTHS = (128, 256, 512, 1024, 2048, 4096, 8192, 11520)
# (H, W): every height at W = 128 (pitch2 = 48, no XCD remap), every width at H = 512 (remap; tails at pitch2 = 144,
# 272, 2064, 2896), and single columns on 512 threads with a remap and a tail
COLS_CASES = [(h, 128) for h in COLS_HEIGHTS] + [(512, w) for w in COLS_WIDTHS[1:]] + [(8184, 1024)]
COLS_JOBS = 2

# (t, h, w, floats past a 16-byte boundary)
ROUTE_CASES = [(2, 512, 128, 0), (2, 1024, 256, 0), (2, 2048, 128, 0), (2, 4096, 128, 0), (1, 8184, 128, 0)] + \
              [(1, 512, w, 0) for w in (512, 1024, 2048, 4096, 8192, 11520)] + [(1, 8184, 1024, 0), (2, 512, 128, 1)]
DISCARDED = (2, 512, 256)
CHUNKS = (5, 512, 256)
RAW_SHAPE = (3, 512, 1024)
# (dtype name, mean_zero); every one with a gain
RAW_CASES = [("uint8", True), ("uint8", False), ("int16", True), ("int16", False)]
RAW_HOT = ("u8", 8.0)  # hot_reference.hot_movie's kind and the threshold
FP16 = (2, 512, 128)


def case_id(case):
    return "x".join(str(v) for v in case[:3]) + ("-offset" if len(case) > 3 and case[3] else "")


def cols_input(H, W):
    """The column pass's input of a table case: complex N(0, 1) in both components, COLS_JOBS jobs of different
    data, columns 0 .. W/4 + 1 (the pair-wide kernels read W/4 + 1 as the partner of W/4), fp32 pairs."""
    r = np.random.default_rng([H, W, 17])
    return r.standard_normal((COLS_JOBS, H, W // 4 + 2, 2)).astype(F32)


def case_frames(t, h, w, other=False):
    """White noise N(0, 2^2) plus an offset of 3 (the DC bin, the kept and the discarded band all carry signal), fp32
    (t, h, w).  `other`: different data of the same kind (the partner of a one-frame case)."""
    g = torch.Generator().manual_seed(t * 7919 + h * 31 + w + (104729 if other else 0))
    return torch.randn(t, h, w, generator=g) * 2.0 + 3.0


@functools.lru_cache(maxsize=2)
def frames_reference(t, h, w):
    """(frames fp32, crop64 of them) of a table case, computed once."""
    x = case_frames(t, h, w)
    return x, crop64(x)


def raw_case(dtype_name):
    """(raw (t, h, w) torch, gain (h, w) torch) of RAW_SHAPE."""
    import kernel_harness as kh

    t, h, w = RAW_SHAPE
    dtype = getattr(torch, dtype_name)
    return kh.raw_movie(t, h, w, dtype, seed=900 + h + (1 if dtype == torch.int16 else 0)), kh.gain(h, w)


def raw_reference(raw, gain, mu):
    """-> (v float64 (t, h, w) = condition_float64 with the fp32 means `mu`, crop64(v), per-frame L2 of the
    conditioning roundings)."""
    from rigid_reference import condition_float64, conditioning_error

    raw, gain = np.asarray(raw), np.asarray(gain)
    v = condition_float64(raw, gain, mu)
    cond = np.array([np.linalg.norm(conditioning_error(raw[f], gain, mu[f])) for f in range(raw.shape[0])])
    return v, crop64(torch.from_numpy(v)), cond


@functools.lru_cache(maxsize=1)
def hot_case():
    """The hot-pixel movie of RAW_SHAPE: (raw, gain, hot64 of the float64 products, x) -- no pixel undecided."""
    import hot_reference as hr

    kind, thr = RAW_HOT
    raw, gain, _ = hr.hot_movie(kind, RAW_SHAPE)
    x = hr.product64(raw, gain)
    return raw, gain, hr.assert_decided(x, thr), x


def hot_reference_frames(raw, gain, ref, x, mu):
    """The hot case against the fp32 means `mu` after replacement: -> (crop64 of replaced - mu, per frame ||c|| of
    the transformed (unreplaced) conditioned samples, `extra` (conditioning), `hot`, fwd_more)."""
    import hot_reference as hr
    from rigid_reference import conditioning_error

    t, h, w = x.shape
    mu = np.asarray(mu, dtype=np.float64)
    want = crop64(torch.from_numpy(ref.replaced - mu[:, None, None]))
    c_norm = np.array([np.linalg.norm(x[f] - mu[f]) for f in range(t)])
    e_r = hr.replacement_error64(ref, x, RAW_HOT[1])
    f_of = ref.keys // (h * w)
    rows, n_in_row = np.unique(ref.keys // w, return_counts=True)
    n_row = n_in_row[np.searchsorted(rows, ref.keys // w)]
    extra, hot, more = [], [], 0.0
    for f in range(t):
        m = f_of == f
        hf, more = hot_terms(e_r[m], (ref.r - ref.v)[m], n_row[m], w)
        hot.append(hf)
        extra.append(np.linalg.norm(conditioning_error(raw[f], gain, mu[f])))
    return want, c_norm, np.array(extra), np.array(hot), more
