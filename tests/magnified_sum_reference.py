"""Shared pieces of the magnified-sum tests (tests/test_magnified_sum_host.py, tests/test_magnified_sum.py): a float64
numpy restatement of the rule of csrc/affine_warp_sum.h -- the aligned sum of a movie with the magnification map folded
into the rigid warp, one interpolation per frame -- the error bound the tests hold the kernel to, the exact result of
the whole-pixel case, and the cases the GPU tests run.

The rule.  Output pixel (y, x), frame f, M (2, 2) float64 in (y, x) order, the frame's fp32 pixel shift (sy, sx):

    (py0, px0) = magnification_reference.positions(h, w, M)        py = py0 + float64(sy)      px = px0 + float64(sx)

one rounded float64 add per axis after the unchanged position chain -- numpy evaluates exactly that, so the positions
and the inside / outside decision here carry the kernel's bits.  A position outside [0, h - 1] x [0, w - 1] contributes
exactly 0; otherwise the value is magnification_reference's: floor, the fractions rounded to fp32 once, the Keys
weights (A = -0.75) of those fractions and the 16 edge-clamped taps, here in float64.  The sum over the frames is taken
in float64.  The pixel shift of an Angstrom field value L at spacing ps is the canonical one of
tests/rigid_reference.py: the correctly rounded fp32 quotient fp32(L) / fp32(ps).

The bound.  With u = 2^-24 and v_f the float64 value of frame f at a pixel:

  - one frame: the kernel's value v^_f is affine::pixel's, so |v^_f - v_f| <= B_f = bound_factor(ty, tx) * a_f, where
    bound_factor is magnification_reference's (the fp32 weights' error, the fraction's rounding, the two nested fp32
    dot products) and a_f = max |tap| over the 16 taps of THIS pixel: the derivation there uses nothing of the image
    but that every tap's magnitude is at most the factor it multiplies by.  B_f = 0 where the frame contributes 0:
    both sides give exactly 0 there.
  - the sum: the kernel adds in fp32, s^_0 = v^_0 (0 + v is exact) and s^_k = fl(s^_{k-1} + v^_k) for k = 1 .. t - 1,
    each add within u of its exact result relatively: |s^_k - (s^_{k-1} + v^_k)| <= u |s^_{k-1} + v^_k|.  With
    S_k = v_0 + ... + v_k the reference's partial sum and E_k a bound on |s^_k - S_k|:
        E_0 = B_0,      E_k = E_{k-1} + B_k + u (|S_k| + E_{k-1} + B_k)
    since |s^_{k-1} + v^_k| <= |S_k| + E_{k-1} + B_k.  E_{t-1} is the bound: the frames' bounds, plus u times the
    magnitude of the running partial sum over the (at most t - 1) rounded adds, that magnitude taken with its own
    uncertainty so that nothing of the kernel's output enters.

Nothing in it comes from a kernel's output, and nothing is tuned."""

from __future__ import annotations

import numpy as np

import magnification_reference as mr
from rigid_reference import F32, _cubic_weights

U = mr.U

# (major_scale, minor_scale, major_axis_angle in degrees) of the general GPU cases and their (t, h, w)
PARAMETERS = ((1.02, 0.98, 30.0), (1.1, 0.9, 117.0))
SHAPES = ((1, 4, 4),        # the smallest frame the entry point takes
          (1, 61, 67),      # smaller than one tile, odd
          (3, 130, 257),    # one past tile multiples on both axes
          (5, 64, 64),      # exactly one tile, five frames in the accumulator
          (2, 1030, 70))    # many tile rows
MAX_SHIFT = 20.0  # |shift| of the general cases, pixels


def pixel_shifts(field, ps):
    """(2, t, 1, 1) Angstrom field (any float dtype) -> (t, 2) fp32 pixel shifts (y, x): the canonical rule, the
    correctly rounded quotient fp32(L) / fp32(ps) (numpy divides fp32 by fp32 exactly so)."""
    lattice = np.asarray(field, dtype=np.float64)[:, :, 0, 0].astype(F32)
    return np.ascontiguousarray((lattice / F32(ps)).astype(F32).T)


def case_field(t, ps, seed=0, max_shift=MAX_SHIFT):
    """A (2, t, 1, 1) fp32 Angstrom field with fractional pixel shifts up to `max_shift` px: the same for every
    caller."""
    rng = np.random.default_rng([int(seed), t, int(round(ps * 1000))])
    px = rng.uniform(-max_shift, max_shift, size=(2, t)).astype(F32)
    return (px * F32(ps)).astype(F32)[:, :, None, None]


def positions(h, w, m, sy, sx):
    """(py, px), each (h, w) float64, of a frame shifted by the fp32 (sy, sx): the rule's operation order."""
    py0, px0 = mr.positions(h, w, m)
    return py0 + np.float64(F32(sy)), px0 + np.float64(F32(sx))


def inside_mask(py, px, h, w):
    return (py >= 0) & (py <= h - 1) & (px >= 0) & (px <= w - 1)


def frame_value(frame, m, sy, sx):
    """One (h, w) frame (taken as its float64 value) -> (value float64, bound float64, inside bool), each (h, w):
    the frame's contribution, B_f of the module's docstring (0 outside) and the inside mask."""
    img = np.asarray(frame, dtype=np.float64)
    h, w = img.shape
    py, px = positions(h, w, m, sy, sx)
    inside = inside_mask(py, px, h, w)
    # outside pixels are evaluated at a harmless position and masked: their floor may be far outside any index range
    fly, flx = np.floor(np.where(inside, py, 0.0)), np.floor(np.where(inside, px, 0.0))
    ty = (np.where(inside, py, 0.0) - fly).astype(F32)
    tx = (np.where(inside, px, 0.0) - flx).astype(F32)
    k = np.arange(4)
    iy = np.clip(fly.astype(np.int64)[..., None] - 1 + k, 0, h - 1)
    ix = np.clip(flx.astype(np.int64)[..., None] - 1 + k, 0, w - 1)
    wy, wx = _cubic_weights(ty.ravel()).reshape(h, w, 4), _cubic_weights(tx.ravel()).reshape(h, w, 4)
    out, amax = np.zeros((h, w)), np.zeros((h, w))
    for i in range(4):
        for j in range(4):
            tap = img[iy[..., i], ix[..., j]]
            out += wy[..., i] * wx[..., j] * tap
            amax = np.maximum(amax, np.abs(tap))
    bound = mr.bound_factor(ty, tx) * amax
    return np.where(inside, out, 0.0), np.where(inside, bound, 0.0), inside


def magnified_sum(stack, m, shifts_px):
    """(t, h, w) stack, M, (t, 2) fp32 pixel shifts -> (sum float64 (h, w), bound float64 (h, w) = E_{t-1},
    frames float64 (t, h, w), frame bounds (t, h, w), inside (t, h, w) bool)."""
    stack = np.asarray(stack)
    t, h, w = stack.shape
    shifts_px = np.asarray(shifts_px, dtype=F32)
    assert shifts_px.shape == (t, 2)
    vals, bnds, ins = np.zeros((t, h, w)), np.zeros((t, h, w)), np.zeros((t, h, w), bool)
    for f in range(t):
        vals[f], bnds[f], ins[f] = frame_value(stack[f], m, shifts_px[f, 0], shifts_px[f, 1])
    total, err = vals[0].copy(), bnds[0].copy()
    for f in range(1, t):
        total = total + vals[f]
        err = err + bnds[f] + U * (np.abs(total) + err + bnds[f])
    return total, err, vals, bnds, ins


def sequential_sum(frames):
    """((0 + v_0) + v_1) + ... in fp32, in frame order: the kernel's accumulator."""
    acc = np.zeros(frames.shape[1:], dtype=F32)
    for f in frames:
        acc = (acc + f.astype(F32)).astype(F32)
    return acc


def shifted_zero_outside(stack, shifts):
    """The frames of the fp32 (t, h, w) stack shifted by whole pixels, out[f][y][x] = stack[f][y + sy][x + sx] and 0
    outside the frame: what identity M gives exactly (weights (0, 1, 0, 0), the other taps exact zeros)."""
    stack = np.asarray(stack, dtype=F32)
    t, h, w = stack.shape
    out = np.zeros_like(stack)
    for f, (sy, sx) in enumerate(np.asarray(shifts)):
        sy, sx = int(sy), int(sx)
        assert sy == shifts[f][0] and sx == shifts[f][1]
        y0, y1, x0, x1 = max(0, -sy), min(h, h - sy), max(0, -sx), min(w, w - sx)
        if y0 < y1 and x0 < x1:
            out[f, y0:y1, x0:x1] = stack[f, y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out
