"""Shared pieces of the Fourier-shift / exposure-sum tests (tests/test_fourier_reference_host.py and
tests/test_fourier_kernels_float64.py): the operations in float64 by their definitions, the error bounds derived
from the arithmetic, and the case tables both files run.

Sign convention: ``fourier_shift64(x, s)`` multiplies the spectrum by exp(-2 pi i (fy sy + fx sx)), which moves the
content by +s; ``correct_motion_fast(image, field)`` applies s = -field (the frame is shifted by -field).

Nothing here is measured on a kernel.  The constants are the unit roundoff u = 2^-24 of fp32, counts of roundings
read off the expressions, Higham's FFT error bound (Accuracy and Stability of Numerical Algorithms, 2nd ed.,
section 24.1, Theorem 24.2) and the accuracy csrc/mc_common.h states for mc_sincos.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
F32 = np.float32
SINCOS_KERNEL = 1e-6    # csrc/mc_common.h: mc_sincos, "~1e-6 absolute for |ang| < 1e5"
SINCOS_LIBM = 2 * U     # a correctly-to-one-ulp sinf / cosf of a value <= 1 (the CPU oracle's)
CAP = 10.0              # per-pixel cap over the rms bound (see bounds())
MAX_OVER_RMS = 8.0      # what the host test asserts of the fp32 reference's own error on every table case


# ------------------------------------------------------------------ the operations, float64


def _t64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().to(torch.float64)
    return torch.from_numpy(np.asarray(x, dtype=np.float64))


def ramp64(h, w, sy, sx):
    """exp(-2 pi i (fy sy + fx sx)) on the rfft2 grid of an (h, w) frame, complex128 (h, w // 2 + 1)."""
    fy = torch.fft.fftfreq(h, dtype=torch.float64)[:, None]
    fx = torch.fft.rfftfreq(w, dtype=torch.float64)[None, :]
    ang = -2.0 * math.pi * (fy * float(sy) + fx * float(sx))
    return torch.complex(torch.cos(ang), torch.sin(ang))


def fourier_shift64(frames, shifts):
    """irfft2(rfft2(x_f) exp(-2 pi i (fy sy_f + fx sx_f)), s=(h, w)) per frame, float64 / complex128; fy =
    fftfreq(h), fx = rfftfreq(w).  `frames` (t, h, w) of any real dtype (taken at its float64 value), `shifts`
    (t, 2) rows (sy, sx) in pixels.  Even and odd h, w.  For even w the Nyquist column is multiplied by the complex
    ramp value like any other bin and irfft2 drops what is not Hermitian (its imaginary part after the column
    transform) -- the rule of the library the project follows."""
    x = _t64(frames)
    s = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    t, h, w = x.shape
    assert s.shape[0] == t, (s.shape, x.shape)
    out = torch.empty_like(x)
    for f in range(t):
        out[f] = torch.fft.irfft2(torch.fft.rfft2(x[f]) * ramp64(h, w, s[f, 0], s[f, 1]), s=(h, w))
    return out


_A, _B, _C = 0.24499, -1.6649, 2.8141


def voltage_scale(voltage):
    return 1.0 if voltage >= 300 else (0.8 if voltage >= 200 else 0.75)


def exposure_exponents64(t, h, w, pixel_size, pre, dose, voltage):
    """The pieces of the exposure filter in float64: (E (t, h, w//2+1), k (h, w//2+1)) with k = max(|k| /
    pixel_size, 1e-6) in 1/Angstrom, N_c = (0.24499 k^-1.6649 + 2.8141) scale, N_f = pre + dose (f + 1) and
    E_f = -1/2 N_f / N_c, so that q_f = exp(E_f)."""
    fy = torch.fft.fftfreq(h, dtype=torch.float64)[:, None]
    fx = torch.fft.rfftfreq(w, dtype=torch.float64)[None, :]
    k = torch.clamp(torch.sqrt(fy * fy + fx * fx) / float(pixel_size), min=1e-6)
    ncrit = (_A * k ** _B + _C) * voltage_scale(voltage)
    nf = float(pre) + float(dose) * torch.arange(1, t + 1, dtype=torch.float64)
    return -0.5 * nf[:, None, None] / ncrit[None], k


def exposure_weights64(t, h, w, pixel_size, pre, dose, voltage):
    """q_f / sqrt(sum_f q_f^2) on the rfft2 grid, float64 (t, h, w // 2 + 1): the filter of
    oracle/thirdparty_semantics.dose_weight_movie."""
    E, _ = exposure_exponents64(t, h, w, pixel_size, pre, dose, voltage)
    q = torch.exp(E)
    return q / torch.sqrt((q * q).sum(0, keepdim=True))


def shift_sums64(frames, shifts=None, pixel_size=None, pre=0.0, dose=None, voltage=300.0):
    """The plain and the exposure-weighted sum of the shifted frames BY THE DEFINITION, frame by frame: y_f =
    fourier_shift64(x_f, s_f) (x_f itself without `shifts`), plain = sum_f y_f, and with a `dose` d_f =
    irfft2(w_f rfft2(y_f)), dw = sum_f d_f.  No sum is ever taken of spectra.  Returns a dict: plain, dw (None
    without a dose), and the per-frame L2 norms the bounds are relative to, norm_y (t,) and norm_d (t,)."""
    x = _t64(frames)
    t, h, w = x.shape
    y = x if shifts is None else fourier_shift64(x, shifts)
    res = {"plain": y.sum(0), "dw": None, "norm_y": np.array([float(torch.linalg.norm(y[f])) for f in range(t)]),
           "norm_d": None}
    if dose is not None:
        wts = exposure_weights64(t, h, w, pixel_size, pre, dose, voltage)
        dw = torch.zeros((h, w), dtype=torch.float64)
        nd = []
        for f in range(t):
            d = torch.fft.irfft2(wts[f] * torch.fft.rfft2(y[f]), s=(h, w))
            nd.append(float(torch.linalg.norm(d)))
            dw += d
        res["dw"], res["norm_d"] = dw, np.array(nd)
    return res


# ------------------------------------------------------------------ the bounds


GAMMA = lambda n: n * U / (1 - n * U)
MU = U                                        # a twiddle rounded from float64 to fp32: |w^ - w| <= u |w| = u
ETA = MU + GAMMA(4) * (math.sqrt(2) + MU)     # Higham Thm 24.2: one radix-2 level, ~6.66 u
C_MUL = MU + math.sqrt(2) * GAMMA(2)          # a complex multiply by an fp32-rounded factor of modulus ~1, ~3.83 u
ANGLE_ROUNDINGS = 6


def radix_cost(r):
    """Relative L2 error one pass of radix r adds to a line (in absolute units, not in u).  A power of two is
    log2(r) nested radix-2 levels with the inter-pass twiddle in the first: log2(r) eta.  Any other radix: the
    inter-pass twiddle multiply (C_MUL) and an r-point DFT whose every output is at worst a direct sum of r
    products with fp32-rounded constants -- per output (MU + sqrt(2) gamma_2 + gamma_(r-1)) sum_j |x_j| <= the same
    times sqrt(r) ||x||; r outputs give sqrt(r) of that in L2, and ||DFT x|| = sqrt(r) ||x||, so the relative error
    is sqrt(r) (MU + sqrt(2) gamma_2 + gamma_(r-1)).  A factored butterfly (12 = 4 x 3, 24 = 8 x 3, 10 = 2 x 5) has
    fewer operations per output than the direct sum."""
    if r & (r - 1) == 0:
        return int(math.log2(r)) * ETA
    return C_MUL + math.sqrt(r) * (MU + math.sqrt(2) * GAMMA(2) + GAMMA(r - 1))


def smooth_radix_list(n):
    """The passes csrc/mc_fft.h::smooth_radix gives a mixed-radix line: 4092 -> 31, 11, 12; 8184 -> 31, 11, 24;
    2880 -> 8, 8, 9, 5; 5760 -> 8, 8, 9, 10."""
    def pick(rem):
        for r in (31, 13, 11, 7):
            if rem % r == 0:
                return r
        if rem in (24, 12):
            return rem
        for r in (8, 4, 9, 10, 5, 3, 2):
            if rem % r == 0:
                return r
        raise ValueError(f"{n} is not a smooth length")
    out, rem = [], n
    while rem > 1:
        out.append(pick(rem))
        rem //= out[-1]
    return out


def prime_factors(n):
    out, p = [], 2
    while n > 1:
        while n % p == 0:
            out.append(p)
            n //= p
        p += 1
    return out


def _pow2(n):
    return n > 0 and n & (n - 1) == 0


def _fft_cost(n):
    """One complex transform of a length the kernels transform directly."""
    return int(math.log2(n)) * ETA if _pow2(n) else sum(radix_cost(r) for r in smooth_radix_list(n))


def _line_cost(n, direction, keep=0):
    """One complex line of the pruned engine as plan.line_plan lays it out: a direct mixed-radix line, or chirp-z --
    chirp multiply, FFT_M, multiply by the filter spectrum, inverse FFT_M, chirp multiply.  Every chirp-z stage's
    error is relative to the norm of the M-point vector it works on; behind the filter that norm is at most
    beta ||x|| (beta = max |FFT_M(b)|, b the wrapped conjugate chirp), errors made before the filter pass through it
    amplified by at most beta as well, and the n wanted outputs have norm sqrt(n) ||x||: the stage errors add up
    and are multiplied by kappa = beta / sqrt(n), computed from the plan's own float64-built table."""
    from torch_motion_correction_amd import plan

    line, keepalive = plan.line_plan(n, direction, torch.device("cpu"), keep)
    if len(keepalive) == 1:  # direct line
        assert line.M == n and n in plan.DIRECT_LINE_LENGTHS and plan.USE_DIRECT_LINES
        return _fft_cost(n), "direct"
    m = int(line.M)
    bs = keepalive[2].double()
    beta = float(torch.sqrt(bs[:, 0] ** 2 + bs[:, 1] ** 2).max()) * m
    kappa = max(1.0, beta / math.sqrt(n))
    return kappa * (3 * C_MUL + 2 * _fft_cost(m)), f"chirp-z M={m}"


def transform_cost(h, w, layout):
    """Relative L2 error of ONE forward and ONE inverse 2-D real transform of an (h, w) frame, first order: the
    passes are unitary up to scale, so their relative errors add.  -> (cost, {axis: kind of line}).

      row_major  csrc/full_fft.hip, full_sums.hip: rows as a packed complex line of w / 2 points plus the pack / unpack
                 butterfly (one more level, eta), columns of h points; powers of two cost log2 levels
                 (Higham), the K3 lengths their smooth_radix_list.
      pruned     xc_rows_fwd*.hip, xc_cols.hip / xcg_*.hip: the same for native power-of-two lines; otherwise plan.line_plan's
                 line of row_line_length(w) points (packed for even w, unpacked for odd w) and of h points,
                 forward with the output pruning the engine asks for.
      polyphase  polyphase.hip: the pruned engine on (h, w / 2) and one radix-2 butterfly each way.
      pocketfft  the CPU library behind the fp32 oracle: a pass per prime factor of each axis.
    """
    kinds = {}
    if layout == "pocketfft":
        one = sum(radix_cost(p) for p in prime_factors(h)) + sum(radix_cost(p) for p in prime_factors(w))
        return 2 * one, {"rows": "pocketfft", "cols": "pocketfft"}
    if layout == "polyphase":
        c, kinds = transform_cost(h, w // 2, "pruned")
        return c + 2 * ETA, kinds
    if layout == "row_major":
        assert w % 2 == 0
        kinds = {"rows": "row-major", "cols": "row-major"}
        return 2 * (_fft_cost(w // 2) + ETA + _fft_cost(h)), kinds
    assert layout == "pruned", layout
    from torch_motion_correction_amd import plan

    g = plan.full_geometry(h, w)
    pack = ETA if w % 2 == 0 else 0.0
    n_r = plan.row_line_length(w)
    if plan.native_rows(g):
        rows, kinds["rows"] = 2 * (_fft_cost(n_r) + pack), "native"
    else:
        fwd, kf = _line_cost(n_r, -1, plan.row_line_keep(w, g.nkx))
        inv, ki = _line_cost(n_r, +1)
        rows, kinds["rows"] = fwd + inv + 2 * pack, ki
    if plan.native_height(h):
        cols, kinds["cols"] = 2 * _fft_cost(h), "native"
    else:
        fwd, _ = _line_cost(h, -1)
        inv, ki = _line_cost(h, +1)
        cols, kinds["cols"] = fwd + inv, ki
    return rows + cols, kinds


def angle_term(shifts):
    """|fp32 angle - exact angle| of (-2 pi fy) sy + (-2 pi fx) sx, per frame.  Per axis five roundings -- 1 / n to
    fp32, k * (1 / n), the constant -2 pi, its product with the frequency, the product with the shift (an exact fp32
    input) -- each at most u of a partial magnitude <= |2 pi f s| <= pi |s|; then the sum (or the fused
    multiply-add) rounds once, at most u of pi (|sy| + |sx|).  Altogether <= 6 u pi (|sy| + |sx|).  By Parseval a
    phase error of at most d radians in every bin is a relative L2 error of at most d."""
    s = np.abs(np.asarray(shifts, dtype=np.float64).reshape(-1, 2))
    return ANGLE_ROUNDINGS * U * math.pi * (s[:, 0] + s[:, 1])


def exposure_term(t, h, w, pixel_size, pre, dose, voltage):
    """Relative fp32 error of the normalised weight w_f = q_f / sqrt(sum q^2), per frame (its maximum over bins).
    Rounding chain of q_f = expf(N_f * (-0.5 / N_c)):
      k      fy, fx two roundings each (1 / n, the product): 2u; squares 5u; their sum 6u; sqrt 4u; pixel_size to
             fp32 and the division: 6u
      powf   the exponent -1.6649 rounded to fp32 moves k^b by |b ln k| u; the error of k enters as |b| 6u = 10u;
             powf itself one ulp = 2u
      N_c    0.24499 to fp32 and the product 2u, + 2.8141 (rounded, then the sum) 2u, the voltage scale (0.8 to
             fp32, the product) 2u; -0.5 / N_c: u
      N_f    pre, dose to fp32, one product, one sum: 3u; N_f * (-0.5 / N_c): u
    so the exponent E has relative error eps_E = (23 + 1.6649 |ln k|) u and q_f = expf(E) the relative error
    |E| eps_E + 2u (expf: one ulp) -- proportional to 1 + 1/2 N_f / N_c.  The norm sqrt(sum_g q_g^2) carries the
    largest of those over the frames, t adds of non-negative terms (t u / 2 after the root), the root and the
    division or reciprocal-and-multiply: 3u."""
    E, k = exposure_exponents64(t, h, w, pixel_size, pre, dose, voltage)
    eps_e = (23 + abs(_B) * torch.abs(torch.log(k))) * U
    eq = (E.abs() * eps_e[None] + 2 * U)
    per_frame = eq.amax(dim=(1, 2)).numpy()
    return per_frame + eq.amax(dim=0).max().item() + (t / 2 + 3) * U


def bounds(h, w, shifts, layout="row_major", sincos=SINCOS_KERNEL, transforms=1):
    """Relative L2 error of one Fourier-shifted frame against fourier_shift64, per frame of `shifts` ((t, 2), or None
    for no ramp), as a dict of its named terms and their sum 'rel' ((t,) arrays):

      fft     transform_cost(h, w, layout) / (1 - that), times `transforms` round trips
      angle   angle_term(shifts)
      sincos  sqrt(2) * `sincos`: sine and cosine each off by that much (mc_common.h's statement for the kernels,
              one ulp for the oracle's libm)
      ramp    the complex multiply by the ramp value and the 1 / (h w) scale: sqrt(2) gamma_2 + u

    The absolute L2 bound of a frame is rel * ||ref||_2.  The per-pixel cap is CAP = 10 times the rms bound, rel *
    rms(ref): on white noise the error of an fp32 evaluation is itself noise-like, with max / rms between 4.7 and 7.0
    over the table's shapes and shifts; tests/test_fourier_reference_host.py re-measures that ratio on the fp32 CPU
    oracle for every table case and asserts it stays <= MAX_OVER_RMS = 8, so the cap rests on the reference's
    behaviour, never on a kernel's."""
    c, kinds = transform_cost(h, w, layout)
    t = 1 if shifts is None else np.asarray(shifts).reshape(-1, 2).shape[0]
    fft = np.full(t, transforms * c / (1 - c))
    if shifts is None:
        zero = np.zeros(t)
        return {"fft": fft, "angle": zero, "sincos": zero, "ramp": zero + U, "rel": fft + U, "kinds": kinds}
    ang = angle_term(shifts)
    sc = np.full(t, math.sqrt(2) * sincos)
    ramp = np.full(t, math.sqrt(2) * GAMMA(2) + U)
    return {"fft": fft, "angle": ang, "sincos": sc, "ramp": ramp, "rel": fft + ang + sc + ramp, "kinds": kinds}


def sum_l2_bound(rel, norms, chunks=1, extra=0.0):
    """Absolute L2 bound of a sum of t frames: every frame's own error, sum_f rel_f ||ref_f|| (a scalar rel applies
    to all), the register accumulators' t - 1 adds, t u sum_f ||ref_f||, one more add per chunk of frames that
    passes through memory, chunks u sum_f ||ref_f||, and `extra` (an absolute L2 term, e.g. conditioning)."""
    norms = np.asarray(norms, dtype=np.float64)
    t = norms.shape[0]
    return float((np.asarray(rel) * norms).sum() + (t + chunks) * U * norms.sum() + extra)


def measure(got, ref):
    """(L2 error, max |error|, rms error) of `got` against `ref`, float64."""
    d = _t64(got) - _t64(ref)
    return float(torch.linalg.norm(d)), float(d.abs().max()), float(torch.sqrt((d * d).mean()))


# ------------------------------------------------------------------ the cases

# rows (sy, sx): zero, integers, half-integers (the Nyquist bin gets a complex ramp value), small fractional, one
# axis only (swapped axes, the sign of fy above h / 2), large, very large (about 1.2e3 rad at the corner bin)
SHIFT_ROWS = ((0.0, 0.0), (3.0, -7.0), (0.5, -2.5), (1.37, -2.81), (4.3, 0.0), (0.0, -5.7), (40.37, -38.61),
              (-200.25, 180.5))
FILLERS = ((-2.19, 0.63), (2.75, 1.5), (-0.81, -1.93), (1.11, 2.93))  # small fractional, to fill the last launch


def case_shifts(t):
    """(K, 2) fp32 shifts of a case of t frames, K the next multiple of t: launch i applies rows i t .. i t + t - 1."""
    rows = list(SHIFT_ROWS)
    i = 0
    while len(rows) % t:
        rows.append(FILLERS[i])
        i += 1
    return np.array(rows, dtype=F32)


def case_frames(t, h, w, offset=False):
    """White noise N(0, 1), or the suite's usual stack N(5, 2^2) with `offset` (DC leakage), fp32 (t, h, w)."""
    g = torch.Generator().manual_seed(t * 7919 + h * 31 + w + (1 if offset else 0))
    x = torch.randn(t, h, w, generator=g)
    return x * 2.0 + 5.0 if offset else x


# (t, h, w, offset input)
ROW_MAJOR_SHIFT = [(3, 256, 64, False), (3, 256, 64, True), (2, 512, 128, False), (2, 1024, 256, False),
                   (2, 2048, 128, False), (2, 4096, 128, False), (2, 4092, 64, False), (2, 8184, 128, False),
                   (2, 256, 1024, False), (1, 256, 8192, False), (2, 256, 5760, False), (1, 256, 11520, False)]
# (t, h, w, offset input, also with DOSE_COLUMN_MAJOR off)
FUSED = [(5, 256, 256, True, False), (5, 4096, 128, False, True), (5, 4092, 64, False, True),
         (4, 8184, 128, False, False), (3, 256, 5760, False, False)]
# (pixel size, dose per frame, pre-exposure, kV)
EXPOSURES = [(1.0, 1.5, 0.0, 300.0), (1.3, 0.8, 2.0, 200.0), (0.5, 0.9, 1.0, 120.0)]
# (t, h, w, offset input, USE_DIRECT_LINES, layout, kind of (rows, columns) line, with the exposure sum).
# (2, 96, 7000) was meant to reach the chirp-z length 5120; its full spectrum does not fit the pruned engine's row
# line (plan.full_geometry raises), so fourier_shift takes the polyphase form on (96, 3500) with M = 4096 -- it
# stays, asserted as what it is -- and (2, 96, 5000) (a row line of 2500 points, 2 n - 1 = 4999 <= 5120) is the
# case that runs M = 5120.
PRUNED = [(2, 256, 256, True, True, "pruned", ("native", "native"), True),
          (2, 64, 600, False, True, "pruned", ("chirp-z M=1024", "native"), True),
          (2, 100, 66, False, True, "pruned", ("chirp-z M=128", "chirp-z M=256"), True),
          (2, 121, 135, False, True, "pruned", ("chirp-z M=512", "chirp-z M=256"), True),
          (2, 2880, 64, False, True, "pruned", ("native", "direct"), False),
          (2, 2880, 64, False, False, "pruned", ("native", "chirp-z M=8192"), False),
          (2, 96, 7000, False, True, "polyphase", ("chirp-z M=4096", "chirp-z M=256"), False),
          (2, 96, 5000, False, True, "pruned", ("chirp-z M=5120", "chirp-z M=256"), False)]
# (t, h, w, offset input, forced)
POLYPHASE = [(3, 256, 512, True, True), (2, 90, 132, False, True), (1, 256, 16384, False, False)]
RAW = [(3, 512, 1024), (3, 4092, 128)]
FP16 = (3, 512, 512)


@functools.lru_cache(maxsize=4)
def shifted_reference(t, h, w, offset, launch):
    """(frames fp32, shifts fp32 (t, 2), fourier_shift64 of them) of launch `launch` of a case; computed once."""
    x = case_frames(t, h, w, offset)
    s = case_shifts(t)[launch * t:(launch + 1) * t]
    return x, s, fourier_shift64(x, s)


def launches(t):
    return len(case_shifts(t)) // t
