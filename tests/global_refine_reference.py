"""Float64 numpy restatement of the iterative sub-pixel whole-frame alignment (refine_global_motion).

TEST INFRASTRUCTURE ONLY.  There is no reference implementation of this estimator (the reference's example calls a
``refine_alignment`` the package never shipped), so the definition is restated here, independently of the HIP path:
fp32 inputs, float64 arithmetic, numpy's FFT.  The mask, the filters and the normalisation are the oracle's
(oracle.motion), evaluated as the oracle evaluates them and widened to float64.

Definition, on S_f = rfft2(normalised frame * mask) * band * B-envelope and shifts s (t, 2) px (y, x):
  start    s = the integer estimate against the reference frame (first maximum, wrap-around rule `p if p <= n//2
           else p - n`), or the caller's;
  per iteration
    G_f   = S_f exp(+2 pi i (fy sy_f + fx sx_f))             (the ramp correct_motion_fast applies for the field s)
    REF_f = (sum_g G_g - G_f) / (t - 1)
    c_f   = irfft2(conj(REF_f) G_f);  p_f = first maximum, wrapped;  parabola offsets of _apply_sub_pixel_refinement
            (estimate_motion_xc.py:465-481, its `!=` guards) from the three samples per axis taken CIRCULARLY
    r_f   = p_f + offsets;   s_f += (t - 1)/t r_f;   s -= s_ref   (the reference frame's row exactly 0)
  stop after the iteration with max_f max(|r_y|, |r_x|) < threshold.
"""

from __future__ import annotations

import numpy as np
import torch

from oracle import motion as om


def filtered_spectra(movie, pixel_spacing, b_factor=500, frequency_range=(300, 10)):
    """(t, h, w//2+1) complex128 filtered spectra of an fp32 (t, h, w) movie."""
    movie = torch.as_tensor(movie).float().cpu()
    _, h, w = movie.shape
    box = movie[:, int(0.25 * h):int(0.75 * h), int(0.25 * w):int(0.75 * w)].double()
    mean, std = box.mean(), box.std()  # normalize_image (utils.py:49-84) in float64
    mask, benv, band = om._filters((h, w), pixel_spacing, b_factor, frequency_range)
    x = ((movie.double() - mean) / std * mask.double()).numpy()
    return np.fft.rfft2(x) * (band.double() * benv.double()).numpy()


def wrap(p, n):
    return p if p <= n // 2 else p - n


def parabola_offset(v0, v1, v2):
    """estimate_motion_xc.py:465-481: no offset when the outer samples are equal."""
    if v2 != v0:
        return type(v0)(0.5) * (v0 - v2) / (v0 - 2 * v1 + v2)
    return 0.0


def residual(cc):
    """(ry, rx, oy, ox) of one correlation map: wrapped first maximum + circular parabola offsets, and the offsets."""
    h, w = cc.shape
    py, px = divmod(int(np.argmax(cc)), w)
    oy = parabola_offset(cc[(py - 1) % h, px], cc[py, px], cc[(py + 1) % h, px])
    ox = parabola_offset(cc[py, (px - 1) % w], cc[py, px], cc[py, (px + 1) % w])
    return wrap(py, h) + oy, wrap(px, w) + ox, oy, ox


def frame_index(reference_frame, t):
    r = int(reference_frame)
    if not -t <= r < t:
        raise IndexError(f"index {r} is out of bounds for dimension 0 with size {t}")
    return r % t


def integer_shifts(S, shape, ref):
    t = S.shape[0]
    s = np.zeros((t, 2))
    for f in range(t):
        if f == ref:
            continue
        cc = np.fft.irfft2(np.conj(S[ref]) * S[f], s=shape)
        py, px = divmod(int(np.argmax(cc)), shape[1])
        s[f] = wrap(py, shape[0]), wrap(px, shape[1])
    return s


FAULTS = ("own frame", "sign", "reference row", "stale", "window offset")


def refine_shifts(S, shape, reference_frame=None, start=None, max_iterations=10, threshold=0.01, damping=None,
                  residuals=None, dtype=np.float64, fault=None):
    """-> (shifts (t, 2) float64 px, history [max |r| per iteration], offsets [(t, 2) parabola offsets per iteration]).
    `damping`: the update factor, default (t - 1)/t.  `residuals`: a list that receives r (t, 2) of every iteration.
    `dtype`: np.float32 runs every statement of the estimator in fp32 (complex64 spectra, numpy's fp32 FFT): the fp32
    stand-in of the host tests.  `fault`: one of FAULTS, a deliberately wrong chain for the tests that must reject it
    ('own frame': the current frame stays in its own reference; 'sign': the x residual is applied with the opposite
    sign; 'reference row': no re-centring; 'stale': the frame after the reference frame is ramped with the shifts of
    the previous iteration; 'window offset' belongs to the patch form and changes nothing here)."""
    assert fault is None or fault in FAULTS, fault
    real = np.dtype(dtype).type
    t = S.shape[0]
    h, w = shape
    ref = frame_index(t // 2 if reference_frame is None else reference_frame, t)
    if t == 1:
        return np.zeros((1, 2)), [], []
    if real is not np.float64:
        S = np.asarray(S).astype(np.complex64)
    s = (integer_shifts(S, shape, ref) if start is None else np.array(start, dtype=np.float64)).astype(real)
    fy, fx = np.fft.fftfreq(h)[:, None].astype(real), np.fft.rfftfreq(w)[None, :].astype(real)
    damp = (real(t - 1) / real(t) if real is not np.float64 else (t - 1) / t) if damping is None else damping
    history, offsets = [], []
    prev = s
    for _ in range(max_iterations):
        used = s
        if fault == "stale":
            used = s.copy()
            used[(ref + 1) % t] = prev[(ref + 1) % t]
        prev = s
        G = S * np.exp(2j * np.pi * (fy[None] * used[:, 0, None, None] + fx[None] * used[:, 1, None, None]))
        A = G.sum(0)
        r, off = np.zeros((t, 2), dtype=real), np.zeros((t, 2), dtype=real)
        for f in range(t):
            REF = A / t if fault == "own frame" else (A - G[f]) / (t - 1)
            cc = np.fft.irfft2(np.conj(REF) * G[f], s=shape)
            assert cc.dtype == real
            r[f, 0], r[f, 1], off[f, 0], off[f, 1] = residual(cc)
        step = damp * r
        if fault == "sign":
            step[:, 1] = -step[:, 1]
        s = s + step
        if fault != "reference row":
            s = s - s[ref]
            s[ref] = 0.0
        assert s.dtype == real
        history.append(float(np.abs(r).max()))
        offsets.append(off)
        if residuals is not None:
            residuals.append(r)
        if history[-1] < threshold:
            break
    return s, history, offsets


def refine_global_motion(movie, pixel_spacing, deformation_field=None, reference_frame=None, b_factor=500,
                         frequency_range=(300, 10), max_iterations=10, convergence_threshold=0.01,
                         return_history=False, return_offsets=False):
    """The restated estimator with the public function's arguments -> (2, t, 1, 1) float64 field in Angstrom."""
    movie = torch.as_tensor(movie)
    t, h, w = movie.shape
    frame_index(t // 2 if reference_frame is None else reference_frame, t)
    if t == 1:
        out = [torch.zeros((2, 1, 1, 1), dtype=torch.float64), [], []]
    else:
        S = filtered_spectra(movie, pixel_spacing, b_factor, frequency_range)
        start = None
        if deformation_field is not None:
            start = (torch.as_tensor(deformation_field).double()[:, :, 0, 0].T / pixel_spacing).numpy()
        s, hist, offs = refine_shifts(S, (h, w), reference_frame, start, max_iterations, convergence_threshold)
        out = [torch.from_numpy(s * pixel_spacing).T[:, :, None, None].contiguous(), hist, offs]
    keep = [True, return_history, return_offsets]
    res = tuple(o for o, k in zip(out, keep) if k)
    return res[0] if len(res) == 1 else res


def planted_movie(t, h, w, drift_y, drift_x, noise, seed=0, band=(0.01, 0.12)):
    """Band-limited periodic texture (unit variance), Fourier-shifted by the planted fractional drifts (frame f shows
    the texture displaced by +drift[f]), plus white noise of `noise` sigma.  -> (fp32 movie (t, h, w), float64
    texture (h, w))."""
    rng = np.random.default_rng(seed)
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.rfftfreq(w)[None, :]
    rad = np.sqrt(fy ** 2 + fx ** 2)
    spec = np.fft.rfft2(rng.standard_normal((h, w))) * ((rad >= band[0]) & (rad <= band[1]))
    tex = np.fft.irfft2(spec, s=(h, w))
    spec = spec / tex.std()
    tex = tex / tex.std()
    dy, dx = np.asarray(drift_y, dtype=np.float64), np.asarray(drift_x, dtype=np.float64)
    ramp = np.exp(-2j * np.pi * (fy[None] * dy[:, None, None] + fx[None] * dx[:, None, None]))
    frames = np.fft.irfft2(spec[None] * ramp, s=(h, w)) + noise * rng.standard_normal((t, h, w))
    return torch.from_numpy(frames.astype(np.float32)), tex
