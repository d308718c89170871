"""A float64 reference of the deformation-field warp (mc_warp_frames_t: csrc/warp_field.hip with warp_field_plan,
warp_field3, warp_field_slow and the route rule; csrc/warp_field_fallback.hip with warp_main, warp_field2; the
tables of csrc/field_tables.hip) driven with a hand-made (t, 2, GH, GW) Angstrom lattice, the cases the
GPU tests run (tests/test_field_kernels_float64.py) and the host emulation of the documented dispatch rules
(tests/test_field_reference_host.py).  Built on tests/rigid_reference.py.

What is restated in fp32 and what is float64.  The reference project's coordinate chain is the specification and
those three objects reproduce it operation by operation wherever FMA contraction is off.  Those parts are restated here in
numpy fp32, every operation rounded on its own, and are bit-reproducible by construction:

  axis tables (warp_axis_tables)  u = _grid_chain(fp32(fp32(p / (n - 1)) * (G - 1)), G); taps
                                  reflect(floor(u) - 1 + k); weights = ATen's Horner forms of fp32(u - floor(u))
  E table (warp_etab)             E[f][c][R][x] = ((c0 L0 + c1 L1) + c2 L2) + c3 L3 along x

The pixel shift s = dot4(ycoef, E rows) / ps may contract to FMA in the kernels, so it is an INTERVAL here:
the float64 value of the dot product of the fp32 coefficients and E values over float64(fp32(ps)), and a bound

  es = (4.01 u M / ps + u (|s| + 4.01 u M / ps)) (1 + 2^-20),   u = 2^-24,  M = sum_k |c_k e_k|:

the four products are each rounded (<= u |c_k e_k|, together <= u M) or fused (no rounding); the three sums are
each one rounding of a partial sum of magnitude <= M (1 + 3u): 3 u M (1 + 3u); 4.01 covers the second-order
terms.  The quotient by ps is one more rounding, u of its own magnitude <= |s| + (dot error) / ps (the kernels'
div_invariant IS the correctly rounded quotient; with ps = 1 there is no division and the bound only has slack).
es is exactly 0 where M is 0, i.e. where every contributing E value is 0: the shift is then exactly 0 in any
evaluation order.  (Subnormal products are not bounded by u |c e|; lattices here are 0 or >= 1e-3.)

From the interval the reference derives per axis the two extreme fp32 coordinates c_lo = fp32(p + (s - es')),
c_hi = fp32(p + (s + es')) -- es' = es + 2^-50 (|p| + |s|) where es > 0, which absorbs the float64 rounding of the
sum so that c_lo <= fp32(p + s_kernel) <= c_hi by monotonicity of rounding -- and u = _grid_chain(c, n) in fp32,
which is monotonic as well: u_lo <= u_kernel <= u_hi.  Per axis there are three situations:

  u_lo == u_hi               one candidate (the common case)
  u_hi == nextafter(u_lo)    two candidates, u_lo and u_hi
  further apart              (small |c| only: fp32 steps finer than es) one candidate, the midpoint m in float64,
                             with the half width r = (u_hi - u_lo) / 2 as a coordinate uncertainty

A pixel has up to 2 x 2 candidates (y, x).  Each is sampled in float64 (bicubic A = -0.75 from the fraction of u,
border padding by clipped taps) and bounded by the rigid kernels' bound 32 u mag + wterm (test_rigid_kernels_
float64.py) [+ the resampled conditioning error for raw movies] plus, for midpoint candidates, the coordinate term

  ry Dy + rx Dx + 1/2 * 24.75 V (ry^2 + rx^2) + 17.64 V ry rx + (32 u * 5.8 + 350 u) V (ry + rx)

  Dy = sum_ij |wy'_i| |wx_j| |v_ij| >= |d out / d uy| at the candidate (wy' the derivative of the Keys weights),
  Dx likewise; V = max |v| of the frame.  out(uy, ux) is C1 (cubic convolution is, also across cells and with
  clipped taps) with piecewise second derivatives |w''| <= 4.5 (near: 7.5 x - 4.5 on [0, 1]; far: 7.5 - 4.5 x on
  [1, 2]), so |d2 out / d uy2| <= 4 * 4.5 * sum|wx| V <= 18 * 1.375 V = 24.75 V: the Taylor remainder.  The mixed
  term uses |w'| <= 1.35 / 0.75 (near / far), sum |w'| <= 4.2: 4.2^2 V ry rx.  The last term lets the rounding
  bound itself move over the interval.  mag = sum_ij |wy_i| |wx_j| |v_ij| is Lipschitz in uy with sum_i |wy'_i| *
  sum_j |wx_j| * V <= 4.2 * 1.375 V <= 5.8 V.  wterm = sum_ij (|wy_i| ex_j + ey_i |wx_j| + ey_i ex_j) |v_ij| with
  e = cubic_weight_error: e_far = ((3x + 6) x + 3) u has |e'| = (6x + 6) u <= 18 u on [1, 2], e_near = ((3x + 1) x +
  2.2) u has |e'| = (6x + 1) u <= 7 u on [0, 1], so sum_i |ey'_i| <= 2 * 18 u + 2 * 7 u = 50 u; sum_j ex_j <= 2 * 27 u
  + 2 * 6.2 u = 66.4 u.  |d wterm / d uy| <= V (4.2 * 66.4 u + 50 u * 1.375 + 50 u * 66.4 u) < 348 u V <= 350 u V,
  and the same in ux.

Zero rule.  `inside` is tested on c as the kernels do.  A pixel whose candidates c_lo / c_hi (either axis) disagree
is ON THE BORDER: the kernel may give exactly 0 or a value within the bound of one of the un-zeroed candidates,
nothing else.  A pixel outside for both is exactly 0; all others are non-zero exactly where the reference is.
"""

from __future__ import annotations

import numpy as np

from rigid_reference import F32, _cubic_weights, _grid_chain, cubic_weight_error

ULP = 2.0 ** -24
TILE_H, TILE_W = 32, 256  # RIGID_WAVES * RIGID_ROWS x RIGID_LANES * 4
GW_MG = 6
GW3_EROWS = 6
PIXEL_SPACINGS = (1.0, 0.83, 1.3)


# ------------------------------------------------------------------ the strict fp32 parts


def horner_weights_f32(t):
    """cubic_coeffs of warp_common.h under contract(off): ATen's Horner forms, every operation rounded to fp32."""
    t = np.asarray(t, dtype=F32)
    A = F32(-0.75)
    a5, a8, a4 = F32(5) * A, F32(8) * A, F32(4) * A
    p2, p3 = A + F32(2), A + F32(3)

    def far(x):
        return ((A * x - a5) * x + a8) * x - a4

    def near(x):
        return (p2 * x - p3) * x * x + F32(1)

    out = np.stack([far(t + F32(1)), near(t), near(F32(1) - t), far(F32(2) - t)], axis=-1)
    assert out.dtype == F32
    return out


def reflect_index(i, size):
    i = np.asarray(i, dtype=np.int64)
    span = size - 1
    a = np.abs(i)
    flips = a // span
    extra = a - flips * span
    return np.clip(np.where(flips & 1, span - extra, extra), 0, size - 1)


def coordinate_tables(coord, n, G):
    """Taps (m, 4) int64 and fp32 weights (m, 4) of the lattice upsample at fp32 coordinates `coord` of an axis
    of n pixels over G nodes (warp_axis_tables with p = coord; warp_pixel_shifts_at)."""
    c = np.asarray(coord, dtype=F32)
    interp = (c / F32(n - 1)).astype(F32) * F32(G - 1)
    u = _grid_chain(interp, G)
    fl = np.floor(u)
    coef = horner_weights_f32((u - fl).astype(F32))
    tap = reflect_index(fl.astype(np.int64)[:, None] - 1 + np.arange(4)[None, :], G)
    return tap, coef


def axis_tables(n, G):
    return coordinate_tables(np.arange(n, dtype=F32), n, G)


def e_table(lattice, w):
    """(t, 2, GH, GW) fp32 lattice -> E (t, 2, GH, w) fp32, the stated order, separate roundings."""
    L = np.asarray(lattice, dtype=F32)
    tap, c = axis_tables(w, L.shape[-1])
    g = [L[..., tap[:, k]] for k in range(4)]
    e = ((c[:, 0] * g[0] + c[:, 1] * g[1]) + c[:, 2] * g[2]) + c[:, 3] * g[3]
    assert e.dtype == F32
    return e


# ------------------------------------------------------------------ the shift interval


def shift_interval(lattice, h, w, ps, x_pass_error=False):
    """-> (s, es), both (t, 2, h, w) float64: the pixel shift [px] and its bound (module docstring).
    `x_pass_error`: the evaluation does not take the E table from warp_etab's stated order but forms the x pass
    itself in some fp32 order (ATen's grid_sample; warp_pixel_shifts_at's direct 16-tap form): each of its
    E values and each of this module's is then off the exact one by <= 4.01 u sum_j |cx_j L_j| (four products,
    three sums), which reaches the dot product through |c_k|: es gains 2 * 4.01 u sum_k |c_k| sum_j |cx_j L_kj| / ps,
    (1 + u) for the quotient's rounding of it."""
    L = np.asarray(lattice, dtype=F32)
    E = e_table(L, w).astype(np.float64)
    ytap, ycoef = axis_tables(h, L.shape[-2])
    yc = ycoef.astype(np.float64)
    psd = float(F32(ps))
    dot = np.zeros(E.shape[:2] + (h, w))
    M = np.zeros_like(dot)
    for k in range(4):
        term = yc[:, k, None] * E[:, :, ytap[:, k], :]
        dot += term
        M += np.abs(term)
    s = dot / psd
    de = 4.01 * ULP * M / psd
    es = (de + ULP * (np.abs(s) + de)) * (1 + 2.0 ** -20)
    if x_pass_error:
        xtap, xc = axis_tables(w, L.shape[-1])
        Mx = sum(np.abs(xc[:, j].astype(np.float64) * L[..., xtap[:, j]].astype(np.float64)) for j in range(4))
        M2 = sum(np.abs(yc[:, k, None]) * Mx[:, :, ytap[:, k], :] for k in range(4))
        es = es + 2 * 4.01 * ULP * M2 / psd * (1 + ULP) * (1 + 2.0 ** -20)
    es[M == 0] = 0.0
    return s, es


def shift_at(lattice2, h, w, ps, coords):
    """warp_pixel_shifts_at: one (2, GH, GW) lattice at fp32 (m, 2) yx pixel coordinates -> (s, es) (m, 2) float64.
    The kernel takes no E table: per lattice row a 4-term x dot product of the lattice values (error
    <= 4.01 u Mx_k, Mx_k = sum_j |cx_j L_kj|), then the 4-term y dot product of those (its own roundings
    <= 4.01 u sum_k |cy_k| (Mx_k + 4.01 u Mx_k), the rows' errors through |cy_k|: 4.01 u M2), M2 = sum_kj
    |cy_k cx_j L_kj|: together <= 8.03 u M2, then the quotient's rounding as in shift_interval."""
    L = np.asarray(lattice2, dtype=F32).astype(np.float64)
    co = np.asarray(coords, dtype=F32)
    ytap, yc = coordinate_tables(co[:, 0], h, L.shape[-2])
    xtap, xc = coordinate_tables(co[:, 1], w, L.shape[-1])
    yc, xc = yc.astype(np.float64), xc.astype(np.float64)
    psd = float(F32(ps))
    dot, M2 = np.zeros((co.shape[0], 2)), np.zeros((co.shape[0], 2))
    for k in range(4):
        for j in range(4):
            term = (yc[:, k] * xc[:, j])[:, None] * L[:, ytap[:, k], xtap[:, j]].T
            dot += term
            M2 += np.abs(term)
    s = dot / psd
    de = 8.03 * ULP * M2 / psd
    es = (de + ULP * (np.abs(s) + de)) * (1 + 2.0 ** -20)
    es[M2 == 0] = 0.0
    return s, es


def dot4_f32(c, e, fused):
    """((c0 e0 + c1 e1) + c2 e2) + c3 e3 on the host, operation by operation in fp32; `fused`: every
    multiply-add that can contract does (fma(c3, e3, fma(c2, e2, fma(c1, e1, c0 e0)))), emulated in float64 --
    exact for the product, one rounding of the sum."""
    c, e = np.asarray(c, dtype=F32), np.asarray(e, dtype=F32)
    if not fused:
        return ((c[..., 0] * e[..., 0] + c[..., 1] * e[..., 1]) + c[..., 2] * e[..., 2]) + c[..., 3] * e[..., 3]
    acc = c[..., 0] * e[..., 0]
    for k in range(1, 4):
        acc = (c[..., k].astype(np.float64) * e[..., k].astype(np.float64) + acc.astype(np.float64)).astype(F32)
    return acc


# ------------------------------------------------------------------ coordinate candidates


def _axis_candidates(p, s, es, n):
    """Per pixel of one axis -> dict with fl (2, ...) int64 / t (2, ...) float64 fraction of the two candidates,
    two (bool: the second candidate differs), r (half width, 0 unless the midpoint is used), inside_lo/hi."""
    pad = np.where(es > 0, 2.0 ** -50 * (np.abs(p) + np.abs(s)), 0.0)
    c_lo = (p + (s - (es + pad))).astype(F32)
    c_hi = (p + (s + (es + pad))).astype(F32)
    top = F32(n) - F32(1)
    in_lo = (c_lo >= F32(0)) & (c_lo <= top)
    in_hi = (c_hi >= F32(0)) & (c_hi <= top)
    u_lo, u_hi = _grid_chain(c_lo, n), _grid_chain(c_hi, n)
    assert bool((u_lo <= u_hi).all())
    same = u_lo == u_hi
    adjacent = ~same & (np.nextafter(u_lo, F32(np.inf)) == u_hi)
    wide = ~same & ~adjacent
    fl = np.stack([np.floor(u_lo), np.floor(u_hi)])
    t = np.stack([(u_lo - fl[0]).astype(F32), (u_hi - fl[1]).astype(F32)]).astype(np.float64)  # the kernels' fp32 fraction
    mid = 0.5 * (u_lo.astype(np.float64) + u_hi.astype(np.float64))
    mfl = np.floor(mid)
    fl[0] = np.where(wide, mfl, fl[0])
    t[0] = np.where(wide, mid - mfl, t[0])
    r = np.where(wide, 0.5 * (u_hi.astype(np.float64) - u_lo.astype(np.float64)), 0.0)
    return {"fl": fl.astype(np.int64), "t": t, "two": adjacent, "r": r, "in_lo": in_lo, "in_hi": in_hi}


def _cubic_weight_derivatives(t):
    """|d w_k / d t| of the four Keys weights, (m, 4) float64."""
    A = -0.75

    def near(x):
        return np.abs((3 * (A + 2) * x - 2 * (A + 3)) * x)

    def far(x):
        return np.abs((3 * A * x - 10 * A) * x + 8 * A)

    return np.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], axis=-1)


def _sample(maps, f, fly, ty, flx, tx, ry, rx):
    """Float64 bicubic samples of frame maps at flat pixel lists.  maps = (v, err or None), each (t, h, w)
    float64; f, fly, flx int64 (m,); ty, tx float64 fractions; ry, rx half widths.  -> (value, bound)."""
    v, err = maps
    h, w = v.shape[-2:]
    wy, wx = _cubic_weights(ty), _cubic_weights(tx)
    ay, ax = np.abs(wy), np.abs(wx)
    ey, ex = ay + cubic_weight_error(ty), ax + cubic_weight_error(tx)
    coord = bool((ry > 0).any() or (rx > 0).any())
    if coord:
        dy, dx = _cubic_weight_derivatives(ty), _cubic_weight_derivatives(tx)
    m = f.shape[0]
    val, mag, wt, er, Dy, Dx = (np.zeros(m) for _ in range(6))
    for i in range(4):
        iy = np.clip(fly - 1 + i, 0, h - 1)
        for j in range(4):
            ix = np.clip(flx - 1 + j, 0, w - 1)
            s = v[f, iy, ix]
            a = np.abs(s)
            val += wy[:, i] * wx[:, j] * s
            mag += ay[:, i] * ax[:, j] * a
            wt += ey[:, i] * ex[:, j] * a
            if err is not None:
                er += ay[:, i] * ax[:, j] * err[f, iy, ix]
            if coord:
                Dy += dy[:, i] * ax[:, j] * a
                Dx += ay[:, i] * dx[:, j] * a
    bound = 32 * ULP * mag + (wt - mag) + er
    if coord:
        V = np.abs(v).reshape(v.shape[0], -1).max(1)[f]
        bound = bound + (ry * Dy + rx * Dx + 0.5 * 24.75 * V * (ry * ry + rx * rx) + 17.64 * V * ry * rx
                         + (32 * ULP * 5.8 + 350 * ULP) * V * (ry + rx))
    return val, bound


class FieldReference:
    """What a kernel's frames must satisfy.  vals / bounds: (4, t, h, w) candidates (y candidate a, x candidate b
    at index 2 a + b; an unused slot repeats candidate 0); zero: pixels outside for every candidate (exactly 0);
    border: pixels whose candidates disagree on `inside`; center / radius: one interval per pixel that contains
    every accepted value (what a frame sum is bounded with)."""

    def __init__(self, vals, bounds, zero, border, s, es, midpoint=None):
        self.zero, self.border, self.s, self.es = zero, border, s, es
        self.midpoint = midpoint  # pixels with a midpoint candidate (a coordinate term in their bound)
        vals = np.where(zero, 0.0, vals)
        bounds = np.where(zero, 0.0, bounds)
        self.vals, self.bounds = vals, bounds
        lo, hi = (vals - bounds).min(0), (vals + bounds).max(0)
        lo, hi = np.where(border, np.minimum(lo, 0.0), lo), np.where(border, np.maximum(hi, 0.0), hi)
        self.center, self.radius = 0.5 * (lo + hi), 0.5 * (hi - lo)

    def check(self, got, what):
        """-> worst |got - candidate| / bound (the best candidate of each pixel); raises on a miss."""
        got = np.asarray(got, dtype=np.float64)
        assert got.shape == self.zero.shape, (got.shape, self.zero.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.abs(got[None] - self.vals)
            ok = (d <= self.bounds).any(0)  # False for NaN
            ratio = np.where(d == 0, 0.0, d / self.bounds).min(0)
        zero_ok = got == 0
        ok = np.where(self.zero, zero_ok, ok & (~zero_ok | (self.vals == 0).any(0)))  # non-zero where the reference is
        ok = np.where(self.border, ok | zero_ok, ok)
        ok &= ~np.isnan(got)
        if not bool(ok.all()):
            bad = np.argwhere(~ok)
            b = tuple(bad[0])
            raise AssertionError(
                f"{what}: {len(bad)} pixels outside every candidate, first (frame, row, col) "
                f"{[tuple(int(v) for v in x) for x in bad[:8]]}; at {b}: got {got[b]!r}, candidates "
                f"{self.vals[(slice(None),) + b].tolist()} bounds {self.bounds[(slice(None),) + b].tolist()} "
                f"zero {bool(self.zero[b])} border {bool(self.border[b])} shift (y, x) {self.s[b[0], :, b[1], b[2]].tolist()} "
                f"+- {self.es[b[0], :, b[1], b[2]].tolist()}")
        ratio = np.nan_to_num(np.where(self.zero | (self.border & zero_ok), 0.0, ratio), nan=0.0, posinf=0.0)
        self.worst = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))  # (frame, row, col)
        self.worst_plain = float(np.where(self.midpoint, 0.0, ratio).max()) if self.midpoint is not None else None
        return float(ratio.max())


def coordinate_candidates(lattice, h, w, ps, x_pass_error=False):
    """-> (cy, cx, zero, border, s, es): the per-axis candidates and the zero / on-border masks (t, h, w)."""
    t = np.asarray(lattice).shape[0]
    s, es = shift_interval(lattice, h, w, ps, x_pass_error)
    py = np.broadcast_to(np.arange(h, dtype=np.float64)[None, :, None], (t, h, w))
    px = np.broadcast_to(np.arange(w, dtype=np.float64)[None, None, :], (t, h, w))
    cy = _axis_candidates(py, s[:, 0], es[:, 0], h)
    cx = _axis_candidates(px, s[:, 1], es[:, 1], w)
    out_y, out_x = ~cy["in_lo"] & ~cy["in_hi"], ~cx["in_lo"] & ~cx["in_hi"]
    zero = out_y | out_x
    inside = cy["in_lo"] & cy["in_hi"] & cx["in_lo"] & cx["in_hi"]
    border = ~zero & ~inside
    return cy, cx, zero, border, s, es


def field_reference(frames, lattice, ps, err=None, x_pass_error=False):
    """frames (t, h, w) (taken as float64 values), lattice (t, 2, GH, GW) fp32 Angstrom, ps -> FieldReference.
    `err`: (t, h, w) per-sample error bound of the frames (raw conditioning), resampled into the bound."""
    v = np.asarray(frames, dtype=np.float64)
    t, h, w = v.shape
    cy, cx, zero, border, s, es = coordinate_candidates(lattice, h, w, ps, x_pass_error)
    maps = (v, None if err is None else np.asarray(err, dtype=np.float64))
    vals, bounds = np.zeros((4, t, h, w)), np.zeros((4, t, h, w))
    for a in (0, 1):
        for b in (0, 1):
            need = ~zero if (a, b) == (0, 0) else ~zero & ((cy["two"] if a else False) | (cx["two"] if b else False))
            # a slot whose own axis has no second candidate repeats the other axis' choice
            f, y, x = np.nonzero(need)
            if f.size:
                ka = np.where(cy["two"][f, y, x], a, 0)
                kb = np.where(cx["two"][f, y, x], b, 0)
                val, bnd = _sample(maps, f, cy["fl"][ka, f, y, x], cy["t"][ka, f, y, x], cx["fl"][kb, f, y, x],
                                   cx["t"][kb, f, y, x], cy["r"][f, y, x], cx["r"][f, y, x])
                vals[2 * a + b][f, y, x], bounds[2 * a + b][f, y, x] = val, bnd
            if (a, b) != (0, 0):
                vals[2 * a + b] = np.where(need, vals[2 * a + b], vals[0])
                bounds[2 * a + b] = np.where(need, bounds[2 * a + b], bounds[0])
    return FieldReference(vals, bounds, zero, border, s, es, (cy["r"] > 0) | (cx["r"] > 0))


def sum_reference(ref, extra_adds=0):
    """(sum of the centres, bound) of a frame sum in fp32: every frame's radius, and t (+ extra_adds) roundings of
    partial sums of magnitude <= sum_f (|centre| + radius) (test_rigid_kernels_float64._sum_bound)."""
    t = ref.center.shape[0]
    return ref.center.sum(0), ref.radius.sum(0) + (t + extra_adds) * ULP * (np.abs(ref.center) + ref.radius).sum(0)


# ------------------------------------------------------------------ documented dispatch rules, on the host


def route_of(h, w, GH, storage="f32", aligned=True):
    """The kernel mc_warp_frames_t / mc_warp_frames_raw take, or 'unsupported' (DESIGN.md section 6)."""
    sparse = 64 * (GH - 1) <= 3 * (h - 1)
    if storage == "f32":
        if w % 4 or not aligned:
            return "warp_main"
        return "warp_field3" if sparse else "warp_field2"
    unit = {"f16": 8, "i16": 8, "u8": 16}[storage]
    return "warp_field3" if (w % unit == 0 and aligned and sparse) else "unsupported"


def tile_plan(lattice, h, w, ps, field3=True):
    """The regularity verdict of warp_field_plan / warp_field2 per (frame, tile, axis), from the rule alone:
    rho = half the range of the lattice nodes the tile's taps touch over ps, n = 3.8 rho + 1.05 in fp32, margin
    ceil(n) when n <= 6 on both axes (and the tile touches <= 6 lattice rows for warp_field3), else irregular.
    -> (mg (t, tiles, 2) int, 0 = irregular; tiles_y, tiles_x)."""
    L = np.asarray(lattice, dtype=F32)
    t, _, GH, GW = L.shape
    ytap, xtap = axis_tables(h, GH)[0], axis_tables(w, GW)[0]
    ty, tx = -(-h // TILE_H), -(-w // TILE_W)
    mg = np.zeros((t, ty * tx, 2), dtype=np.int64)
    for tl in range(ty * tx):
        yt, xt = (tl // tx) * TILE_H, (tl % tx) * TILE_W
        rows = ytap[np.minimum(np.arange(yt, yt + TILE_H), h - 1)]
        cols = xtap[np.minimum(np.arange(xt, xt + TILE_W), w - 1)]
        R0, R1, C0, C1 = rows.min(), rows.max(), cols.min(), cols.max()
        nodes = L[:, :, R0:R1 + 1, C0:C1 + 1].reshape(t, 2, -1)
        rho = (F32(0.5) * (nodes.max(-1) - nodes.min(-1))).astype(F32) / F32(ps)
        n = (F32(3.8) * rho).astype(F32) + F32(1.05)
        regular = (n <= GW_MG).all(-1) & (not field3 or R1 - R0 + 1 <= GW3_EROWS)
        mg[:, tl] = np.where(regular[:, None], np.ceil(n).astype(np.int64), 0)
    return mg, ty, tx


# ------------------------------------------------------------------ lattice families and cases

FAMILIES = ("zero", "integer", "fraction", "smooth2", "smooth3", "smooth4", "smooth5", "smooth6", "rough", "big",
            "beyond", "one_row_col")
# upper end of rho for margin class m is (m - 1.05) / 3.8; the smooth families aim at the middle of their class
_CLASS_RHO = {m: (m - 1.55) / 3.8 for m in (2, 3, 4, 5, 6)}


def family_lattice(name, h, w, GH, GW, ps, rng):
    """One frame's (2, GH, GW) fp32 Angstrom lattice of family `name` (values in px times ps)."""
    const = {"zero": (0.0, 0.0), "integer": (3.0, -5.0), "fraction": (2.37, -1.61), "big": (40.5, -77.25),
             "beyond": (h + 0.5, 3.25), "one_row_col": (h - 1.5, -(w - 1.5))}
    if name in const:
        px = np.array(const[name], dtype=F32)[:, None, None] * np.ones((1, GH, GW), dtype=F32)
        return (px * F32(ps)).astype(F32)
    base = rng.uniform(-1, 1, size=(2, GH, GW))
    base = 2 * (base - base.min((1, 2), keepdims=True)) / np.ptp(base, axis=(1, 2), keepdims=True) - 1  # range [-1, 1]
    offset = rng.uniform(-4, 4, size=(2, 1, 1))
    if name == "rough":  # smooth everywhere but around node (0, 0), 6 px away: rho = 3 on the tiles that touch it
        px = 0.1 * base + offset
        px[:, 0, 0] += 6.0
    else:
        px = _CLASS_RHO[int(name[-1])] * base + offset
    return (px * ps).astype(F32)


def case_lattices(case, ps, launch):
    """(t, 2, GH, GW) lattices of launch number `launch` of a case: frame i takes family (launch * t + i) mod 12."""
    t, h, w, GH, GW = case
    rng = np.random.default_rng([t, h, w, GH, GW, launch])
    return np.stack([family_lattice(FAMILIES[(launch * t + i) % len(FAMILIES)], h, w, GH, GW, ps, rng)
                     for i in range(t)])


def case_launches(case):
    """[(launch number, ps)]: enough launch numbers for every family (one for a case of >= 12 frames), and every
    launch number at ps = 1.0 (the UNIT_PS instantiations) AND at one other spacing (0.83 and 1.3 alternate): the
    spacing does not depend on the family, so every family -- the rough one, every margin class, the integer shift
    times ps -- meets both kinds of instantiation in every case."""
    t = case[0]
    n = -(-len(FAMILIES) // t)
    return [(i, ps) for i in range(n) for ps in (1.0, PIXEL_SPACINGS[1 + i % 2])]


# mc_warp_frames_raw_accumulate: storage -> (t, h, w, GH, GW), and the (families of the 6 frames, frames per chunk)
# of its runs: two chunks without an irregular tile-frame, three chunks with some
ACCUM_CASES = {"u8": (6, 96, 528, 5, 4), "i16": (6, 96, 520, 5, 4)}
ACCUM_RUNS = ((("fraction", "smooth2", "smooth4", "integer", "smooth6", "big"), 3),
              (("smooth3", "rough", "zero", "one_row_col", "rough", "smooth5"), 2))
ACCUM_SPACINGS = (1.0, 0.83)


def accumulate_lattices(case, families, ps):
    t, h, w, GH, GW = case
    assert len(families) == t
    rng = np.random.default_rng([t, h, w, len(families[0])])
    return np.stack([family_lattice(f, h, w, GH, GW, ps, rng) for f in families])


# route -> [(t, h, w, GH, GW)]
FIELD_CASES = {
    "warp_main": [(3, 33, 130, 4, 5), (2, 40, 258, 3, 3)],
    "warp_main_unaligned": [(3, 33, 260, 2, 3)],  # `frames` one float past a 16-byte boundary
    "warp_field2": [(3, 33, 260, 8, 5), (2, 64, 520, 20, 30)],
    "warp_field3": [(3, 33, 260, 2, 3),    # last tile row: one pixel row; last tile column: one quad
                    (3, 32, 256, 2, 2),    # exactly one tile
                    (3, 96, 516, 5, 4),
                    (2, 64, 2048, 3, 7),   # 16 tiles: the workgroup-to-tile remap
                    (2, 72, 1536, 3, 4),   # 18 tiles: no remap
                    (130, 33, 260, 2, 3)],  # the second plan block
    "warp_field3_half": [(3, 33, 264, 2, 3), (3, 96, 520, 5, 4), (2, 64, 2048, 3, 7)],
    "warp_field3_u8": [(3, 33, 272, 2, 3), (3, 96, 528, 5, 4), (2, 64, 2048, 3, 7), (130, 33, 272, 2, 3)],
    "warp_field3_i16": [(3, 33, 264, 2, 3), (3, 96, 520, 5, 4), (2, 64, 2048, 3, 7)],
}
CASE_STORAGE = {"warp_main": "f32", "warp_main_unaligned": "f32", "warp_field2": "f32", "warp_field3": "f32",
                "warp_field3_half": "f16", "warp_field3_u8": "u8", "warp_field3_i16": "i16"}
