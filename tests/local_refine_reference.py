"""Float64 numpy restatement of the iterative sub-pixel patch alignment (refine_local_motion).

TEST INFRASTRUCTURE ONLY, built like tests/global_refine_reference.py and independent of the HIP path: fp32 inputs,
float64 arithmetic, numpy's FFT.  The mask, the filters and the field resampling are the oracle's (oracle.motion),
widened to float64; the patch lattice is the host-side integer code of the package (lattice.patch_grid_centers).

Definition, with p the patch side, (cy, cx) the lattice, origin[q] = (cy - p//2, cx - p//2), npatch = gh gw:
  start    s0[f, q] px (y, x): the caller's Angstrom field / pixel spacing, resampled to (t, gh, gw) (Catmull-Rom,
           resample_deformation_field); None: the restated refine_global_motion of the same movie (same b_factor,
           frequency_range, reference_frame, default iteration settings);
  offsets  o[f, q] = clip(rint(s0), -origin, (h - p, w - p) - origin) per axis (rint: halves to even); the window
           of job (f, q) is movie[f, origin + o : origin + o + p];
  spectra  S[f, q] = rfft2((window - mean) / std * mask) * band * B-envelope, mean / std the central-box statistics
           of the whole movie (normalize_image, float64);
  per iteration, per patch q
    G[f]   = S[f, q] exp(+2 pi i (fy (sy - oy) + fx (sx - ox)))
    REF[f] = (sum_g G[g] - G[f]) / (t - 1)
    r[f]   = wrapped first maximum of irfft2(conj(REF[f]) G[f]) + circular parabola offsets
    s[f, q] += (t - 1)/t r[f];   s[:, q] -= s[ref, q]       (the reference frame exactly 0 in every patch)
  stop after the iteration with max over (f, q) of max(|r_y|, |r_x|) < threshold.
"""

from __future__ import annotations

import numpy as np
import torch

import global_refine_reference as gr
from oracle import motion as om
from torch_motion_correction_amd import lattice


def patch_lattice(shape, p):
    """(cy, cx, origin (npatch, 2) int64): centres and window corners, patches in row-major (gy, gx) order."""
    t, h, w = shape
    cy, cx = lattice.patch_grid_centers(t, h, w, p)
    origin = np.stack([np.repeat(cy - p // 2, len(cx)), np.tile(cx - p // 2, len(cy))], axis=1)
    return cy, cx, origin.astype(np.int64)


def window_offsets(s0, shape, p):
    """(t, npatch, 2) int64 offsets of the windows for the (t, npatch, 2) start shifts."""
    _, h, w = shape
    _, _, origin = patch_lattice(shape, p)
    hi = np.array([h - p, w - p]) - origin
    return np.clip(np.rint(np.asarray(s0, dtype=np.float64)), -origin[None], hi[None]).astype(np.int64)


def start_px(deformation_field, pixel_spacing, shape, p):
    """(t, npatch, 2) float64 px start shifts from a (2, nt, nh, nw) Angstrom field."""
    t = shape[0]
    cy, cx, _ = patch_lattice(shape, p)
    field = torch.as_tensor(deformation_field).double().cpu()
    lat = om.resample_deformation_field(field, (t, len(cy), len(cx))).double()  # (2, t, gh, gw)
    return (lat / pixel_spacing).permute(1, 2, 3, 0).reshape(t, -1, 2).numpy()


def patch_spectra(movie, pixel_spacing, p, offsets, b_factor=500, frequency_range=(300, 10)):
    """(t, npatch, p, p//2+1) complex128 filtered spectra of the windows cut at origin + offsets."""
    movie = torch.as_tensor(movie).float().cpu()
    t, h, w = movie.shape
    box = movie[:, int(0.25 * h):int(0.75 * h), int(0.25 * w):int(0.75 * w)].double()
    mean, std = float(box.mean()), float(box.std())  # normalize_image (utils.py:49-84) in float64
    mask, benv, band = om._filters((p, p), pixel_spacing, b_factor, frequency_range)
    mask, filt = mask.double().numpy(), (band.double() * benv.double()).numpy()
    _, _, origin = patch_lattice((t, h, w), p)
    frames = movie.double().numpy()
    S = np.empty((t, len(origin), p, p // 2 + 1), dtype=np.complex128)
    for f in range(t):
        for q, (oy, ox) in enumerate(origin + offsets[f]):
            assert 0 <= oy <= h - p and 0 <= ox <= w - p, (f, q, oy, ox)
            S[f, q] = np.fft.rfft2((frames[f, oy:oy + p, ox:ox + p] - mean) / std * mask) * filt
    return S


def refine_patches(S, p, start, offsets, reference_frame=None, max_iterations=10, threshold=0.01, damping=None,
                   dtype=np.float64, fault=None):
    """-> (shifts (t, npatch, 2) float64 px, history [max |r| per iteration], parabola offsets [(t, npatch, 2) per
    iteration], residuals [(t, npatch, 2) per iteration]).  `damping`: the update factor, default (t - 1)/t.
    `dtype`, `fault`: as global_refine_reference.refine_shifts (np.float32: the fp32 stand-in; a deliberately wrong
    chain); 'window offset' leaves the window offset of patch 0 out of its ramp."""
    assert fault is None or fault in gr.FAULTS, fault
    real = np.dtype(dtype).type
    t, npatch = S.shape[:2]
    ref = gr.frame_index(t // 2 if reference_frame is None else reference_frame, t)
    s = np.array(start, dtype=np.float64).reshape(t, npatch, 2).astype(real)
    if t == 1:
        return np.zeros((1, npatch, 2)), [], [], []
    if real is not np.float64:
        S = np.asarray(S).astype(np.complex64)
    o = np.asarray(offsets, dtype=real)
    fy, fx = np.fft.fftfreq(p)[:, None].astype(real), np.fft.rfftfreq(p)[None, :].astype(real)
    damp = (real(t - 1) / real(t) if real is not np.float64 else (t - 1) / t) if damping is None else damping
    history, parabola, residuals = [], [], []
    prev = s
    for _ in range(max_iterations):
        used = s
        if fault == "stale":
            used = s.copy()
            used[(ref + 1) % t] = prev[(ref + 1) % t]
        prev = s
        r, off = np.zeros((t, npatch, 2), dtype=real), np.zeros((t, npatch, 2), dtype=real)
        for q in range(npatch):
            d = used[:, q] if (fault == "window offset" and q == 0) else used[:, q] - o[:, q]
            G = S[:, q] * np.exp(2j * np.pi * (fy[None] * d[:, 0, None, None] + fx[None] * d[:, 1, None, None]))
            A = G.sum(0)
            for f in range(t):
                REF = A / t if fault == "own frame" else (A - G[f]) / (t - 1)
                cc = np.fft.irfft2(np.conj(REF) * G[f], s=(p, p))
                assert cc.dtype == real
                r[f, q, 0], r[f, q, 1], off[f, q, 0], off[f, q, 1] = gr.residual(cc)
        step = damp * r
        if fault == "sign":
            step[..., 1] = -step[..., 1]
        s = s + step
        if fault != "reference row":
            s = s - s[ref][None]
            s[ref] = 0.0
        assert s.dtype == real
        history.append(float(np.abs(r).max()))
        parabola.append(off)
        residuals.append(r)
        if history[-1] < threshold:
            break
    return s, history, parabola, residuals


def refine_local_motion(movie, pixel_spacing, patch_sidelength=1024, deformation_field=None, reference_frame=None,
                        b_factor=500, frequency_range=(300, 10), max_iterations=10, convergence_threshold=0.01,
                        details=False):
    """The restated estimator with the public function's arguments -> (2, t, gh, gw) float64 field in Angstrom; with
    `details` also a dict of history, parabola offsets, residuals, window offsets and the start."""
    movie = torch.as_tensor(movie)
    shape = tuple(movie.shape)
    t, p = shape[0], int(patch_sidelength)
    gr.frame_index(t // 2 if reference_frame is None else reference_frame, t)
    cy, cx, _ = patch_lattice(shape, p)
    gh, gw = len(cy), len(cx)
    if t == 1:
        field = torch.zeros((2, 1, gh, gw), dtype=torch.float64)
        return (field, dict(history=[], parabola=[], residuals=[])) if details else field
    if deformation_field is None:
        deformation_field = gr.refine_global_motion(movie, pixel_spacing, None, reference_frame, b_factor,
                                                    frequency_range)
    s0 = start_px(deformation_field, pixel_spacing, shape, p)
    o = window_offsets(s0, shape, p)
    S = patch_spectra(movie, pixel_spacing, p, o, b_factor, frequency_range)
    s, hist, par, res = refine_patches(S, p, s0, o, reference_frame, max_iterations, convergence_threshold)
    field = torch.from_numpy((s * pixel_spacing).reshape(t, gh, gw, 2)).permute(3, 0, 1, 2).contiguous()
    if details:
        return field, dict(history=hist, parabola=par, residuals=res, offsets=o, start=s0)
    return field


# ------------------------------------------------------------------ an analytic movie with local motion


def planted_local_movie(t, h, w, rigid, slope, noise, seed=0, band=(0.01, 0.12), waves=36):
    """A movie whose local motion is exact without any resampler.  The texture is a sum of `waves` sinusoids with
    random directions, frequencies in `band` (cycles/px) and phases, of unit variance; frame f shows it at
    n - d_f(n), evaluated in float64, with d_f(n) = rigid[f] + slope[f] * (x - (w - 1)/2) / w: a drift (y and x
    components, px) that varies linearly from the left to the right edge by slope[f] in total.  Because d_f depends
    on x only, every sinusoid separates into a function of y times a function of x and a frame is two matrix
    products.  Plus white noise of `noise` sigma.
    -> (fp32 movie (t, h, w), drift(f, y, x) -> (dy, dx) float64)."""
    rng = np.random.default_rng(seed)
    rad = rng.uniform(band[0], band[1], waves)
    ang = rng.uniform(0.0, np.pi, waves)
    ky, kx = rad * np.sin(ang), rad * np.cos(ang)
    phase = rng.uniform(0.0, 2 * np.pi, waves)
    amp = np.sqrt(2.0 / waves)
    rigid, slope = np.asarray(rigid, dtype=np.float64), np.asarray(slope, dtype=np.float64)
    y, x = np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64)
    u = (x - (w - 1) / 2) / w

    def drift(f, yy, xx):
        uu = (np.asarray(xx, dtype=np.float64) - (w - 1) / 2) / w
        return rigid[f, 0] + slope[f, 0] * uu, rigid[f, 1] + slope[f, 1] * uu

    Y = 2 * np.pi * y[:, None] * ky[None, :]  # (h, waves)
    frames = np.empty((t, h, w))
    for f in range(t):
        dy, dx = rigid[f, 0] + slope[f, 0] * u, rigid[f, 1] + slope[f, 1] * u
        X = 2 * np.pi * (kx[:, None] * (x - dx)[None, :] - ky[:, None] * dy[None, :]) + phase[:, None]  # (waves, w)
        frames[f] = amp * (np.cos(Y) @ np.cos(X) - np.sin(Y) @ np.sin(X))
    frames += noise * rng.standard_normal((t, h, w))
    return torch.from_numpy(frames.astype(np.float32)), drift


def planted_truth(drift, shape, p, reference_frame=None):
    """(t, npatch, 2) planted shifts at the patch centres relative to the reference frame."""
    t = shape[0]
    ref = gr.frame_index(t // 2 if reference_frame is None else reference_frame, t)
    cy, cx, _ = patch_lattice(shape, p)
    yy, xx = np.repeat(cy, len(cx)), np.tile(cx, len(cy))
    d = np.stack([np.stack(drift(f, yy, xx), axis=-1) for f in range(t)])  # (t, npatch, 2)
    return d - d[ref][None]
