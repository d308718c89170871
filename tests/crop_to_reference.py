"""Shared pieces of the tests of Fourier cropping to a given size (tests/test_crop_to_host.py, tests/test_crop_to.py):
the definition in float64 (crop_to64), the error bound derived from the arithmetic, and the case tables.  Everything
here is float64 on the CPU and knows nothing of the package's kernels; nothing is measured on a kernel.  The notation,
the per-line costs and the halving's bound are tests/crop_reference.py's; what that module hard-codes as H/2 and W/2
stands here with two lengths.

The bound.  u = 2^-24, eta = one radix-2 level with fp32-rounded twiddles, _fft_cost(n) the relative L2 error of one
complex n-point line as the kernels factor it (crop_reference's docstring).  The crop is not a round trip: the forward
passes err relative to the norm of what they transform (the whole frame), the crop is a projection, and the inverse
passes err relative to what is left.  So the bound is absolute, one term per side:

  frame   F = DFT2(x) unnormalised, ||F|| = sqrt(H W) ||x|| over the full (Hermitian) spectrum.  The fp32 row pass (a
          packed W/2-point line and the unpack level) and the H-point column pass give F + E,
              ||E|| <= c_fwd sqrt(H W) ||x||,     c_fwd = _fft_cost(W/2) + eta + _fft_cost(H).
          Cropping to -H2/2 <= ky < H2/2, kx <= W2/2 keeps bins (each kept bin once) and the real inverse drops the
          imaginary parts of its DC and Nyquist bins: projections, of norm <= 1, for ANY H2 <= H and W2 <= W.  The
          unnormalised inverse at (H2, W2) multiplies norms by sqrt(H2 W2), and the scale is 1 / (H2 W2).  So E
          reaches the output as at most
              sqrt(H2 W2) / (H2 W2) c_fwd sqrt(H W) ||x|| = A c_fwd ||x||,     A = sqrt(H W / (H2 W2))
          (2 for the halving; 1.5 for 8184 x 11520 -> 5456 x 7680; sqrt(4/3 * 2) for 512 x 256 -> 384 x 128).
          The inverse passes hold the cropped spectrum, whose image is the reference y = crop_to64(x):
              c_inv ||y||,     c_inv = _fft_cost(H2) + _fft_cost(W2/2) + eta (the pack level).
          The scale: the constant 1 / (H2 W2) rounded to fp32 (crop_to64 divides by the exact product) and the
          product with it: 2 u ||y|| (crop_reference.SCALE_FRAME).
              l2 = (A (c_fwd ||x|| + extra) + (c_inv + 2 u) ||y||) / (1 - c_fwd - c_inv)
          `extra`: an absolute L2 error of the INPUT, spread like noise; it passes through the same A.

  cap     per pixel: CAP = 10 times the rms form of the same bound, l2 / sqrt(H2 W2) (crop_reference's rule).

  hot     a raw movie with a hot-pixel list (crop_reference's `hot` paragraph): per list entry the localised input
          errors e_r + 2 eps |dA| (crop_reference.hot_terms), added by the triangle inequality, `fwd_more` = u more in
          c_fwd.  Two factors of that paragraph carry the halving: a perturbation d at one input pixel reaches an
          output pixel through the crop's point response, 1 / (H2 W2) times a sum of at most H2 (W2 + 1) unit
          phasors, modulus <= 1 + 1 / W2; a perturbation p along one row keeps that factor along y and along x
          passes the 1-D crop, whose L2 gain is sqrt(W / W2), so max |.| <= sqrt(W / W2) ||p||_2.  In L2 a localised
          input error passes through A like any other.
              local = (1 + 1 / W2) sqrt(W / W2) hot,     cap = CAP (l2 - A hot) / sqrt(H2 W2) + local
"""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

import crop_reference as cr
from crop_reference import CAP, ETA, SCALE_FRAME, U, _fft_cost, frame_ratios  # noqa: F401


# ------------------------------------------------------------------ the definition


def crop_to64(x, shape):
    """The definition, in float64 on the CPU: rows -h2/2 <= ky < h2/2 (signed; the new Nyquist row from the negative
    side) and columns 0 <= kx <= w2/2 of rfft2(x), inverted at (h2, w2); irfft2's 1 / (h2 w2) is the only scale (the
    c2r ignores the imaginary parts of its DC and Nyquist bins).  One frame at a time."""
    x = x.detach().cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))
    if x.dim() == 3:
        return torch.stack([crop_to64(f, shape) for f in x])
    x = x.double()
    h, w = x.shape
    h2, w2 = shape
    assert h2 % 2 == 0 and w2 % 2 == 0 and 2 <= h2 <= h and 2 <= w2 <= w, (x.shape, shape)
    F = torch.fft.rfft2(x)
    G = torch.cat((F[: h2 // 2, : w2 // 2 + 1], F[h - h2 // 2:, : w2 // 2 + 1]), dim=0)
    return torch.fft.irfft2(G, s=(h2, w2))


def dense_crop_to64(x, shape):
    """The same thing stated independently: dense float64 DFT matrices, no FFT.  F[ky][kx] = sum x exp(-2 pi i (ky y
    / h + kx x / w)) for kx <= w2/2; the rows with signed frequency -h2/2 <= ky < h2/2, each at ky mod h2; c[n][kx] =
    sum over them of F exp(+2 pi i ky n / h2); and the real inverse written out as the cosine series it is,
        y[n][m] = (Re c[n][0] + (-1)^m Re c[n][w2/2] + 2 sum_{0 < kx < w2/2} Re(c[n][kx] exp(2 pi i kx m / w2))) / (h2 w2),
    in which the imaginary parts of the DC and Nyquist columns do not occur."""
    x = np.asarray(x, dtype=np.float64)
    h, w = x.shape
    h2, w2 = shape
    nk = w2 // 2 + 1
    F = np.exp(-2j * np.pi * np.outer(np.arange(h), np.arange(h)) / h) @ x @ \
        np.exp(-2j * np.pi * np.outer(np.arange(w), np.arange(nk)) / w)
    signed = np.arange(-h2 // 2, h2 // 2)
    c = np.exp(2j * np.pi * np.outer(np.arange(h2), signed) / h2) @ F[signed % h]  # (h2, nk)
    m = np.arange(w2)
    y = c[:, :1].real + c[:, -1:].real * (-1.0) ** m[None, :]
    for kx in range(1, w2 // 2):
        y = y + 2.0 * (c[:, kx:kx + 1] * np.exp(2j * np.pi * kx * m / w2)[None, :]).real
    return y / (h2 * w2)


def band_limited_to(h, w, shape, seed, t=None):
    """float64 frames whose spectrum is zero at and beyond the Nyquist frequencies of the (h2, w2) grid."""
    h2, w2 = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((h, w) if t is None else (t, h, w), generator=g, dtype=torch.float64)
    F = torch.fft.rfft2(x)
    F[..., h2 // 2: h - h2 // 2 + 1, :] = 0  # |ky| >= h2/2
    F[..., :, w2 // 2:] = 0  # kx >= w2/2
    return torch.fft.irfft2(F, s=(h, w))


def resampled(x, shape):
    """The exact resampling of a band-limited frame on the (h2, w2) grid over the same field of view, straight from
    its Fourier series: x(y h / h2, x w / w2), times (h w) / (h2 w2) -- the crop keeps the frame's SUM, so a pixel
    holds the counts of the h w / (h2 w2) input pixels it stands for.  Dense float64 sums, no FFT of the output."""
    x = np.asarray(x, dtype=np.float64)
    h, w = x.shape
    h2, w2 = shape
    F = np.fft.fft2(x) / (h * w)
    fy, fx = np.fft.fftfreq(h) * h, np.fft.fftfreq(w) * w  # signed integer frequencies
    ey = np.exp(2j * np.pi * np.outer(np.arange(h2) / h2, fy))  # (h2, h)
    ex = np.exp(2j * np.pi * np.outer(fx, np.arange(w2) / w2))  # (w, w2)
    return (ey @ F @ ex).real * (h * w) / (h2 * w2)


# ------------------------------------------------------------------ the bound


def amplification(h, w, h2, w2):
    """A of the module docstring."""
    return math.sqrt((h * w) / (h2 * w2))


def frame_costs(h, w, h2, w2):
    """(c_fwd, c_inv) of the module docstring."""
    return _fft_cost(w // 2) + ETA + _fft_cost(h), _fft_cost(h2) + _fft_cost(w2 // 2) + ETA


def frame_bound(h, w, h2, w2, x_norm, ref_norm, extra=0.0, fwd_more=0.0, hot=0.0):
    """Absolute L2 bound of one frame cropped from (h, w) to (h2, w2) against crop_to64: ||x||_2 of the frame the
    forward passes transform, ||ref||_2 of its crop, `extra`, `fwd_more`, `hot` as in crop_reference.frame_bound.
    -> dict: fwd (the A c_fwd ||x|| term, higher orders included), l2, cap (per pixel)."""
    c_fwd, c_inv = frame_costs(h, w, h2, w2)
    c_fwd += fwd_more
    a = amplification(h, w, h2, w2)
    amp = 1.0 / (1.0 - c_fwd - c_inv)
    fwd = amp * a * c_fwd * x_norm
    spread = fwd + amp * (a * extra + (c_inv + SCALE_FRAME) * ref_norm)
    local = amp * (1.0 + 1.0 / w2) * math.sqrt(w / w2) * hot
    return {"fwd": fwd, "l2": spread + amp * a * hot, "cap": CAP * spread / math.sqrt(h2 * w2) + local}


def crop_to_scale(h2, w2):
    """The scale mc_full_cols_crop_to applies: float32(1 / (h2 w2)), widened back."""
    return float(np.float32(1.0 / (float(h2) * float(w2))))


def cols_crop_to64(S, H, H2, W2):
    """mc_full_cols_crop_to restated: for each job and each kx <= W2/2, along y, the unnormalised H-point DFT (sign
    -), the rows ky < H2/2 at ky and ky >= H - H2/2 at ky - (H - H2), the unnormalised H2-point DFT (sign +), times
    crop_to_scale.  S (jobs, H, >= W2/2 + 1 columns) -> complex128 (jobs, H2, W2/2 + 1)."""
    z = cr._as_complex(S)[:, :, : W2 // 2 + 1]
    assert z.shape[1] == H
    F = np.fft.fft(z, axis=1)
    G = np.concatenate((F[:, : H2 // 2], F[:, H - H2 // 2:]), axis=1)
    return np.fft.ifft(G, axis=1) * H2 * crop_to_scale(H2, W2)


def cols_bound(H, H2, W2, s_norm, r_norm):
    """crop_reference.cols_bound with two lengths: one column s (H samples) -> r (H2 samples).  Forward error c_H
    sqrt(H) ||s|| in the unnormalised spectrum, projection, unnormalised inverse sqrt(H2), scale: a_col = scale
    sqrt(H H2); the inverse and the product with the (shared, rounded) scale err relative to r.
    -> (l2, cap per complex bin, by its modulus)."""
    c_h, c_h2 = _fft_cost(H), _fft_cost(H2)
    a_col = crop_to_scale(H2, W2) * math.sqrt(H * H2)
    l2 = (a_col * c_h * np.asarray(s_norm) + (c_h2 + cr.SCALE_COLS) * np.asarray(r_norm)) / (1.0 - c_h - c_h2)
    return l2, CAP * l2 / math.sqrt(H2)


def added(b1, b2):
    """The bound of the difference of two results that each lie within their own bound of the same float64 value."""
    return {"l2": b1["l2"] + b2["l2"], "cap": b1["cap"] + b2["cap"]}


# ------------------------------------------------------------------ the cases

# (t, h, w), (h2, w2): the smallest shapes that run each instantiation of the column pass and each new row length
ROUTE_CASES = [((2, 512, 256), (384, 128)),      # mixed-radix output columns from a power-of-two line
               ((2, 4092, 128), (2046, 64)),
               ((1, 8184, 128), (5456, 64)),
               ((1, 8184, 128), (2728, 64)),
               ((1, 4096, 128), (3072, 64)),
               ((2, 512, 5760), (384, 2880)),    # row length 1440
               ((2, 512, 4096), (384, 3072)),    # 1536
               ((2, 512, 11520), (384, 3840)),   # 1920
               ((2, 512, 11520), (384, 7680))]   # 3840
WHOLE_FRAME = ((1, 4092, 5760), (2046, 2880))
EDGES = ((512, 256), (384, 128))
CHUNKS = ((4, 512, 256), (384, 128))
HALVING = (2, 512, 1024)
RAW = ((3, 512, 5760), (384, 2880))
# (dtype name, gain, mean_zero)
RAW_CASES = [("uint8", True, True), ("uint8", True, False), ("int16", True, True), ("int16", True, False),
             ("uint8", False, True)]
RAW_HOT = cr.RAW_HOT
UNSUPPORTED = [((2, 4092, 5760), (3072, 2880)),   # no 4092 -> 3072
               ((2, 8184, 11520), (4092, 7680)),  # the halving of one axis alone
               ((2, 960, 928), (480, 464)),
               ((2, 512, 5760), (384, 1440))]     # no 720-point row line

SHAPES_FOR_FACTORS = [((4092, 5760, 2), (2046, 2880)), ((8184, 11520, 1.5), (5456, 7680)),
                      ((8184, 11520, 3), (2728, 3840)), ((4096, 4096, 4 / 3), (3072, 3072)),
                      ((8184, 11520, 2), (4092, 5760))]


def case_id(case):
    (t, h, w), (h2, w2) = case
    return f"{t}x{h}x{w}-to-{h2}x{w2}"


@functools.lru_cache(maxsize=2)
def frames_reference(shape, out_shape):
    """(frames fp32, crop_to64 of them) of a table case, computed once (crop_reference.case_frames: white noise plus
    an offset, so the DC bin, the kept and the discarded band all carry signal)."""
    x = cr.case_frames(*shape)
    return x, crop_to64(x, out_shape)


def edge_impulses(h, w, h2, w2):
    """[(name, (ky, kx), kept)]: the rows and columns on either side of the crop's edges."""
    return [("ky = h2/2 - 1", (h2 // 2 - 1, 3), True), ("ky = h2/2", (h2 // 2, 3), False),
            ("ky = h - h2/2", (h - h2 // 2, 3), True), ("ky = h - h2/2 - 1", (h - h2 // 2 - 1, 3), False),
            ("kx = w2/2", (5, w2 // 2), True), ("kx = w2/2 + 1", (5, w2 // 2 + 1), False)]


def impulse_frame(h, w, ky, kx, phase=0.7):
    """The real (h, w) frame whose half spectrum is one impulse of modulus h w / 2 and the given phase at (ky, kx)
    (and its Hermitian twin): cos(2 pi (ky y / h + kx x / w) + phase), float64."""
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    return torch.cos(2 * torch.pi * (ky * yy / h + kx * xx / w) + phase)
