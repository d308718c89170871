"""Shared pieces of the rigid-warp route tests (tests/test_rigid_shift_rounding_host.py and
tests/test_rigid_routes.py): the canonical per-frame pixel shift, the cases the GPU tests run, and a
float64 rigid resampler that applies the reference's sampling rule to an exact fp32 shift.

The canonical shift rule.  A rigid (2, t, 1, 1) Angstrom field gives frame f the lattice value L (fp32, the
spline in time at t_f); the warp's pixel shift is the correctly rounded fp32 quotient

    shifts_px = fp32(L) / fp32(ps)

which is what the CPU reference computes (``get_pixel_shifts``: a CPU tensor divided by a Python float is true
division), what the general-field kernel computes, and what the movie pipeline's ``rigid_tail`` computes.  At
an integer node s of a catmull_rom field L = fp32(s * ps) exactly.  Multiplying by fp32(1 / ps) instead rounds
twice and differs in the last bit for some (s, ps): at ps = 0.83 and s = -3 it gives -3 - 2.4e-7, and the
sampling coordinate p + s of pixel p = 3 becomes negative -- a border row or column the reference keeps is
zeroed.
"""

from __future__ import annotations

import numpy as np

F32 = np.float32

# (pixel spacing, integer pixel shifts) the GPU tests use; every spacing != 1 must contain shifts at which the
# two roundings differ (asserted on the host by test_rigid_shift_rounding_host.py)
TABLE_SPACINGS = (1.0, 0.83, 1.06, 1.3, 1.35, 2.5)
FRAME_SPACINGS = (0.83, 1.06, 1.3)
PIPELINE_SPACINGS = (0.83, 1.35)
RAW_SPACINGS = (0.83, 1.3)
# spacings at which fp32(1/ps) is exact enough that both roundings agree for every integer shift
EXACT_RECIPROCAL = (1.0, 2.5)

# shifts (per axis) that separate the two roundings: at 0.83 the reciprocal is more negative for
# -3, -5, -6, -10..-12 and smaller for +3, +5, +6, ...; at 1.06 / 1.3 / 1.35 it is closer to zero for
# +-9, +-13 / +-7, +-14, +-15 / +-13, +-15
SMALL_SHIFTS = (-3, -5, -6, -9, -10, -12, -13, -7, -15, 3, 5, 6, 7, 9, 13, 15, 0)
LARGE_SHIFTS = (-150, 150, -131, 121)


def canonical_shift(s_px, ps):
    """fp32 pixel shift of an integer node shift s_px of a catmull_rom field: fp32(fp32(s * ps) / ps)."""
    L = np.asarray(s_px, dtype=F32) * F32(ps)
    return (L / F32(ps)).astype(F32)


def reciprocal_shift(s_px, ps):
    """What a multiply by the fp32 reciprocal gives (ATen's tensor / python-scalar CUDA kernel)."""
    L = np.asarray(s_px, dtype=F32) * F32(ps)
    return (L * (F32(1.0) / F32(ps))).astype(F32)


def row_dropping_shifts(shifts, ps):
    """The negative integers of `shifts` whose reciprocal quotient is more negative than the true one."""
    s = np.unique(np.asarray(shifts, dtype=np.int64))
    s = s[s < 0]
    return [int(v) for v in s if reciprocal_shift(v, ps) < canonical_shift(v, ps)]


def differing_shifts(shifts, ps):
    s = np.unique(np.asarray(shifts, dtype=np.int64))
    return [int(v) for v in s if reciprocal_shift(v, ps) != canonical_shift(v, ps)]


def _grid_chain(c, n):
    """grid_sample's align_corners=True round trip of an array coordinate, in fp32:
    ((c / (0.5 n - 0.5) - 1) + 1) * ((n - 1) / 2) (array_to_grid_sample, then ATen's un-normalisation)."""
    d = F32(0.5) * F32(n) - F32(0.5)
    g = (c / d).astype(F32) - F32(1)
    return ((g + F32(1)) * ((F32(n) - F32(1)) / F32(2))).astype(F32)


def _cubic_weights(t):
    """Keys cubic convolution weights, A = -0.75 (ATen's bicubic), float64, for fractions t (m,) -> (m, 4)."""
    A = -0.75
    t = t.astype(np.float64)

    def near(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def far(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A

    return np.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], axis=-1)


def _axis_operator(n, s):
    """(n, n) float64 matrix M with out = M @ column for one axis shifted by the fp32 shift s, plus the
    bool mask of output indices whose coordinate p + s lies inside [0, n - 1] (the rest are zero)."""
    p = np.arange(n, dtype=F32)
    c = (p + F32(s)).astype(F32)
    inside = (c >= F32(0)) & (c <= F32(n - 1))
    u = _grid_chain(c, n)
    fl = np.floor(u)
    w = _cubic_weights((u - fl).astype(F32))
    M = np.zeros((n, n), dtype=np.float64)
    base = fl.astype(np.int64) - 1
    for k in range(4):
        idx = np.clip(base + k, 0, n - 1)  # border padding
        np.add.at(M, (np.arange(n), idx), w[:, k])
    M[~inside] = 0.0
    return M, inside


def rigid_resample(frame, sy, sx):
    """One (h, w) frame (any real dtype; taken as its float64 value) shifted by the fp32 pixel shift (sy, sx) with
    the reference's rule: out[y, x] = bicubic(frame)(c_y, c_x), c = fp32(p + s), border padding, zero where c leaves
    [0, n - 1].  Returns (out float64, absolute-weight magnitude sum_ij |wy_i wx_j v_ij| per pixel, float64)."""
    f = np.asarray(frame, dtype=np.float64)
    h, w = f.shape
    My, _ = _axis_operator(h, sy)
    Mx, _ = _axis_operator(w, sx)
    out = My @ f @ Mx.T
    mag = np.abs(My) @ np.abs(f) @ np.abs(Mx).T
    return out, mag


def rigid_resample_stack(stack, shifts_px):
    """(t, h, w) stack and (t, 2) fp32 shifts -> (frames float64, magnitudes float64)."""
    st = np.asarray(stack, dtype=np.float64)
    sh = np.asarray(shifts_px, dtype=F32)
    outs, mags = zip(*(rigid_resample(st[f], sh[f, 0], sh[f, 1]) for f in range(st.shape[0])))
    return np.stack(outs), np.stack(mags)


def coordinate_ulp(h, w):
    """Spacing of fp32 just below max(h, w): one ulp of the largest sampling coordinate."""
    return 2.0 ** (int(np.ceil(np.log2(max(h, w)))) - 1 - 23)


def neighbour_gradient(ref):
    """Largest absolute neighbour difference within each pixel's 5 x 5 footprint (the span of a one-ulp move of
    either coordinate through the bicubic taps), (t, h, w) float64."""
    ref = np.asarray(ref, dtype=np.float64)
    gy = np.zeros_like(ref)
    gx = np.zeros_like(ref)
    gy[..., :-1, :] = np.abs(np.diff(ref, axis=-2))
    gx[..., :, :-1] = np.abs(np.diff(ref, axis=-1))
    g = np.maximum(gy, gx)
    out = g.copy()
    h, w = g.shape[-2:]
    pad = np.pad(g, [(0, 0)] * (g.ndim - 2) + [(2, 2), (2, 2)])
    for dy in range(5):
        for dx in range(5):
            out = np.maximum(out, pad[..., dy:dy + h, dx:dx + w])
    return out
