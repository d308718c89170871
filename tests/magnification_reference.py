"""Shared pieces of the magnification-distortion tests (tests/test_magnification_host.py, tests/test_magnification.py):
a float64 numpy restatement of the rule of csrc/affine_resample.h -- positions, the fill decision, clamped taps, Keys
weights -- the error bound the GPU tests hold the kernel to, and the cases they run.

The rule.  Output pixel (y, x) of an h x w frame, cy = h // 2, cx = w // 2, M (2, 2) float64 in (y, x) order:

    py = (cy + m00 * (y - cy)) + m01 * (x - cx)        px = (cx + m10 * (y - cy)) + m11 * (x - cx)

in float64, every operation rounded on its own, in this order -- numpy evaluates exactly that, so the positions here
carry the bits the kernel's carry.  A position outside [0, h - 1] x [0, w - 1] gives fill_value; otherwise
iy = floor(py), ix = floor(px), the fractions (exact differences in float64) are rounded to fp32, and the output is
sum_ij wy_i wx_j v[clip(iy - 1 + i)][clip(ix - 1 + j)] with the Keys weights, A = -0.75, of those fp32 fractions; here the
weights and the sum are float64.

The bound.  The kernel evaluates the weights in fp32 with ATen's Horner forms (fused or not) and accumulates in fp32:
four products and three sums per tap row, then the same over the four rows.  With u = 2^-24:

  - weights: |fp32 weight - float64 weight| <= e = rigid_reference.cubic_weight_error(t) per tap, absolute;
  - the fraction: the rule rounds it to fp32 and both sides round the same float64 value, so they agree; an independent
    float64 evaluation that does NOT round it (grid_sample in float64, tests/test_magnification_host.py) differs by a
    fraction off by <= u/2 <= u; a weight moves by at most |w'| u with |w'| <= 1.35 on a near tap and <= 0.75 on a far
    one (the derivatives cubic_weight_error quotes): d = (0.75, 1.35, 1.35, 0.75) u is added to e;
  - accumulation: a dot product of 4 terms evaluated ((a + b) + c) + d has every term multiplied by at most
    (1 + u)^4 (its product and three sums; a fused multiply-add only removes a rounding), and the two nested dot
    products give (1 + u)^8 <= 1 + g, g = 8u / (1 - 8u);
  - every tap has magnitude <= vmax = max |image|.

So  |kernel - reference| <= vmax * sum_ij ((|wy_i| + ey_i + d_i) (|wx_j| + ex_j + d_j) (1 + g) - |wy_i| |wx_j|)
per pixel (`bound`): 111 u vmax at fractions of 0 (e sums to 47.4 u and d to 4.2 u per axis, g = 8 u), about 150 u
vmax = 9e-6 vmax at fractions of 0.5.  Nothing in it comes from a kernel's output.
"""

from __future__ import annotations

import numpy as np

from rigid_reference import F32, _cubic_weights, cubic_weight_error

U = 2.0 ** -24
FRACTION_SLOPE = np.array([0.75, 1.35, 1.35, 0.75])  # max |dw/dt| of the far, near, near, far tap

# (major_scale, minor_scale, major_axis_angle in degrees) and the (t, h, w) of the general GPU cases
PARAMETERS = ((1.02, 0.98, 30.0), (1.1, 0.9, 117.0), (0.9, 0.9, 0.0), (1.1, 1.1, 45.0))
SHAPES = ((1, 61, 67),     # smaller than one tile, odd
          (3, 130, 257),   # one past tile multiples on both axes
          (1, 1030, 70))   # many tile rows
EDGE_MARGIN = 1e-9  # no source position of the cases lies this close to 0, h - 1 or w - 1


def matrix(major, minor, angle_degrees):
    """D = major u u^T + minor (I - u u^T), u = (cos, sin) as (x, y), rewritten in (y, x) order; float64 numpy."""
    a = np.deg2rad(np.float64(angle_degrees))
    u = np.array([np.cos(a), np.sin(a)])  # (x, y)
    d = major * np.outer(u, u) + minor * (np.eye(2) - np.outer(u, u))  # (x, y) order
    return d[::-1, ::-1].copy()


def positions(h, w, m):
    """(py, px), each (h, w) float64, in the rule's operation order."""
    m = np.asarray(m, dtype=np.float64)
    cy, cx = h // 2, w // 2
    dy = (np.arange(h, dtype=np.int64) - cy).astype(np.float64)[:, None]
    dx = (np.arange(w, dtype=np.int64) - cx).astype(np.float64)[None, :]
    py = (np.float64(cy) + m[0, 0] * dy) + m[0, 1] * dx
    px = (np.float64(cx) + m[1, 0] * dy) + m[1, 1] * dx
    return py, px


def inside_mask(h, w, m):
    py, px = positions(h, w, m)
    return ~((py < 0) | (py > h - 1) | (px < 0) | (px > w - 1))


def edge_distance(h, w, m):
    """The least distance of a source position's coordinate from 0 and from n - 1 (the fill decision's edges)."""
    py, px = positions(h, w, m)
    return float(min(np.abs(py).min(), np.abs(py - (h - 1)).min(), np.abs(px).min(), np.abs(px - (w - 1)).min()))


def _taps(h, w, m):
    py, px = positions(h, w, m)
    inside = ~((py < 0) | (py > h - 1) | (px < 0) | (px > w - 1))
    fly, flx = np.floor(py), np.floor(px)
    ty, tx = (py - fly).astype(F32), (px - flx).astype(F32)  # exact differences, rounded to fp32 once
    k = np.arange(4)
    iy = np.clip(fly.astype(np.int64)[..., None] - 1 + k, 0, h - 1)  # (h, w, 4)
    ix = np.clip(flx.astype(np.int64)[..., None] - 1 + k, 0, w - 1)
    return inside, iy, ix, ty, tx


def resample(image, m, fill_value=0.0):
    """(h, w) or (t, h, w) image (taken as its float64 value) -> (the reference float64, the bound float64), same
    shape; the bound is 0 where the output is fill_value."""
    img = np.asarray(image, dtype=np.float64)
    stack = img if img.ndim == 3 else img[None]
    t, h, w = stack.shape
    inside, iy, ix, ty, tx = _taps(h, w, m)
    wy, wx = _cubic_weights(ty.ravel()).reshape(h, w, 4), _cubic_weights(tx.ravel()).reshape(h, w, 4)
    out = np.zeros((t, h, w))
    for i in range(4):
        for j in range(4):
            out += (wy[..., i] * wx[..., j])[None] * stack[:, iy[..., i], ix[..., j]]
    out = np.where(inside[None], out, np.float64(fill_value))
    bnd = np.where(inside, bound_factor(ty, tx), 0.0)[None] * np.abs(stack).max(axis=(1, 2), keepdims=True)
    return (out, bnd) if img.ndim == 3 else (out[0], bnd[0])


def bound_factor(ty, tx):
    """sum_ij ((|wy_i| + ey_i + d_i) (|wx_j| + ex_j + d_j) (1 + g) - |wy_i| |wx_j|) for fp32 fractions ty, tx (any
    shape): the bound per unit of max |image| (the module's docstring)."""
    shape = np.shape(ty)
    ty, tx = np.ravel(ty), np.ravel(tx)
    ay, ax = np.abs(_cubic_weights(ty)), np.abs(_cubic_weights(tx))
    ey, ex = ay + cubic_weight_error(ty) + FRACTION_SLOPE * U, ax + cubic_weight_error(tx) + FRACTION_SLOPE * U
    g = 8 * U / (1 - 8 * U)
    return (ey.sum(-1) * ex.sum(-1) * (1 + g) - ay.sum(-1) * ax.sum(-1)).reshape(shape)


def frames(t, h, w, seed=0):
    """Random fp32 frames (t, h, w), normal with standard deviation 2 about 5: the same for every caller."""
    rng = np.random.default_rng([int(seed), t, h, w])
    return (rng.standard_normal((t, h, w)) * 2 + 5).astype(F32)
