"""Shared pieces of tests/test_post_reference_host.py and tests/test_post_kernels_float64.py: the float64 definitions of
the three small kernel families every patch estimate and every field warp passes through -- the leave-one-out reference
spectra (mc_xc_ref_mean_except_current with lattice.leave_one_out_schedule), the temporal smoothing and centring of the
patch field (mc_field_smooth_center), the cubic spline grids (spline.axis_taps with mc_spline_lattice / mc_spline_points,
csrc/field_tables.hip)
and the plan's tables (mc_circle_mask, mc_xc_filter) -- with the error bound of each and the case lists.

TEST INFRASTRUCTURE ONLY: numpy (and torch on the CPU for linspace / searchsorted, the two operations that DEFINE a spline
interval in both code bases) in float64 on the fp32 inputs at their exact value.  Nothing here imports the package's
kernels or spline.py; the fp32 knots, the fp32 coordinate and the fp32 basis matrix are inputs of the definition.  No
constant is measured on a kernel.  u = 2^-24, gamma_k = k u / (1 - k u).

A. REFERENCE SPECTRA   REF64[f] = (1 / (t - 1)) sum_{o != f} (V_o if ref_expo[f, o] == 1 else U_o), complex128, straight
   from the (t, t) table.  The kernel forms, per component, r = fl(fl(fl(T - U_f) + d) * inv):
     T     the t-term fp32 sum of U_o, t - 1 roundings of partial sums:           e_T = gamma_{t-1} sum_o |U_o|
     a     = fl(T - U_f):                                                          e_a = e_T + u (|T64 - U_f| + e_T)
     d     the running sum of fl(V_o - U_o) over the m = |S_f| members carried since the last rebuild (the schedule's
           invariant: the carried set IS S_f), one rounding per difference, m - 1 per partial sum:
                                                                                   e_d = gamma_m sum_{o in S_f} |V_o - U_o|
     b     = fl(a + d):                                                            e_b = e_a + e_d + u (|b64| + e_a + e_d)
     r     = fl(b * inv), inv the fp32 rounding of 1 / (t - 1):      bound = (e_b (1 + u)^2 + gamma_2 |b64|) / (t - 1)
   per element and absolute, every term weighted by the absolute values actually added; b64 = (t - 1) REF64.  Nothing
   is relative to |REF64| (T - U_f cancels).

B. SMOOTHING   window < 3: the copy; else interior mean of x[i - half .. i + half] (odd) / x[i - w/2 + 1 .. i + w/2]
   (even: scipy's kernel sits half a sample late), least-squares line through the first / last `window` samples on
   the edges; with subtract_mean the mean over all 2 t npatch values is subtracted.  The kernel accumulates in double
   and rounds the smoothed value once: u |y| (nothing on the copy route: no arithmetic), plus the double terms
   16 window 2^-53 max|x| (sum, centring, slope and evaluation of the fit, each <= 4 window roundings of values <= max|x|
   times line weights <= 1).  Mean subtraction: the block sum in double (n 2^-53 max|y|), its fp32 rounding u |mean|, the
   fp32 difference u |y - mean|:   u (|y| + |mean| + |y - mean|) + double terms.  That sum, taken alone, is not a
   bound: the kernel takes the mean over the ROUNDED smoothed values, so the average of their n roundings, at most
   u mean_j |y_j|, shifts every output -- on a field with mean near 0 and few values it is the largest term (the
   contract evaluated on the CPU with double accumulation is up to 12 times outside the three-term sum at n = 80).
   With it (window >= 3 only; the copy route rounds nothing):
     bound = u (|y| + mean_j |y_j| + |mean| + |y - mean|) + double terms, times (1 + 8u) for products of two roundings.

C. SPLINE GRIDS   oracle.thirdparty_semantics.cubic_spline_grid_3d restated with explicit padding: single-sample axes
   duplicated, one linearly extrapolated sample per side, interval il = clip(searchsorted(linspace32(0, 1, n), u32,
   right) - 1, 0, n - 2), s = (u32 - knot32[il]) (n - 1), value = sum over the 4 x 4 x 4 padded samples of the products
   of [1, s, s^2, s^3] @ M, all in float64 (M at its fp32 entries: they are the library's constants).
   The kernels get folded fp32 tap weights from the host and run three nested fp32 sums (x, y, t):
     s      u - knot is exact (Sterbenz: knot <= u <= 2 knot for il >= 1, knot = 0 for il = 0); times (n - 1): u |s|
     p_j    s^2 from the rounded s: 3u s^2; s^3 (two products): 5u s^3
     basis  b_k = sum_j p_j M_jk in fp32, any order: e_b[k] = sum_j (c_j + 4) u |p_j| |M_jk|, c = (0, 1, 3, 5)
     fold   lo (il == 0): w1 = fl(b1 + 2 b0), w2 = fl(b2 - b0), w0 = 0; hi (il + 2 == n): w2 = fl(w2 + 2 b3),
            w1 = fl(w1 - b3), w3 = 0: the errors of the parts add (2 b is exact) and every fl adds u |result|
     sums   each level is 4 products and 3 additions: gamma_4 of sum |w d| per level, gamma_12 in all
   bound = [ sum_taps |d| (e_wt |wy wx| + |wt| e_wy |wx| + |wt wy| e_wx) + gamma_12 sum_taps |wt wy wx d| ] (1 + 100u)
   over the 64 taps WITH THE FOLDED WEIGHTS (folding doubles a weight; the folded weights are formed here in float64
   from this module's own basis); the last factor covers products of the <= 50 first-order terms of a path.

D. PLAN TABLES   mask: inside <=> fp32 sqrt(dy^2 + dx^2) < radius (the squared distance is an integer < 2^24: exact);
   d = fp32(scipy's float64 Euclidean distance to the nearest inside pixel); value cos(pi/2 d / s) for 0 < d <= s.
   Inside exactly 1, beyond the ring exactly 0, ring within 6u absolute (xc_reference's docstring: constant, quotient
   and product round, 3u of an angle <= pi/2 = 4.7u, the cosine an ulp).  No inside pixel at all: zeros (mcorr.h).
   filter: fy = fp32(k) * fp32(1 / H), fx likewise, f = sqrt(fy fy + fx fx), every operation rounded to fp32; kept <=>
   low < f <= high in fp32.  Envelope exp(-B (F / ps)^2 / 4) in float64 at the exact frequency F = sqrt((k/H)^2 +
   (kx/W)^2) with the fp32 values of B and ps.  fp32: 1/H and the product 2u, the square 5u, the sum 6u, the root 4u,
   / ps 5u, its square 11u, times B 12u, / 4 exact: the exponent E carries 12u relative, the value 12 |E| u; expf an
   ulp (2u):   bound = (12 |E| + 2) u value.  Excluded bins exactly 0.
"""

from __future__ import annotations

import functools

import numpy as np
import torch
from scipy import ndimage

U = 2.0 ** -24
EPS64 = 2.0 ** -53
F32 = np.float32


def gamma(k):
    return k * U / (1 - k * U)


# ------------------------------------------------------------------ A. reference spectra


def ref_mean64(Uc, Vc, ref_expo):
    """(REF64 (t, n) complex128, bound (t, n, 2) per real / imaginary component) from U, V (t, n) complex128 and the
    (t, t) exponent table."""
    Uc, Vc = np.asarray(Uc, dtype=np.complex128), np.asarray(Vc, dtype=np.complex128)
    t = Uc.shape[0]
    comp = lambda z: np.stack([z.real, z.imag], axis=-1)  # noqa: E731
    u, v = comp(Uc), comp(Vc)
    e_T = gamma(t - 1) * np.abs(u).sum(axis=0)
    T = u.sum(axis=0)
    ref = np.empty_like(Uc)
    bound = np.empty(u.shape)
    for f in range(t):
        members = [o for o in range(t) if o != f and ref_expo[f, o] == 1]
        others = [o for o in range(t) if o != f and ref_expo[f, o] != 1]
        b64 = comp(Vc[members].sum(axis=0) + Uc[others].sum(axis=0))
        ref[f] = (b64[..., 0] + 1j * b64[..., 1]) / (t - 1)
        e_a = e_T + U * (np.abs(T - u[f]) + e_T)
        e_d = gamma(len(members)) * np.abs(v[members] - u[members]).sum(axis=0)
        e_b = e_a + e_d + U * (np.abs(b64) + e_a + e_d)
        bound[f] = (e_b * (1 + U) ** 2 + gamma(2) * np.abs(b64)) / (t - 1)
    return ref, bound


def hand_table(sets):
    """(t, t) table with S_f = sets[f]: 1 on the members, 0 elsewhere, -1 on the diagonal."""
    t = len(sets)
    tab = np.zeros((t, t), dtype=np.int64)
    for f, s in enumerate(sets):
        assert f not in s
        tab[f, sorted(s)] = 1
        tab[f, f] = -1
    return tab


# name -> list of S_f.  'reset': S_3 drops frames 0 and 1 (an eviction in the middle) and grows again afterwards;
# 'member': frame 1 and frame 3 are members of their predecessor's set (the `f not in prev` branch)
HAND_TABLES = {
    "reset": [set(), {0}, {0, 1}, {2}, {2, 3}, {2, 3, 4}],
    "empty": [set()] * 4,
    "full": [set(range(5)) - {f} for f in range(5)],
    "member": [{1, 2}, {0, 2}, {0, 1}, {0, 1, 2, 4}, {0, 1, 2}],
}
SCHEDULE_T = [2, 3, 8, 52, 60]            # lattice.mask_schedule(t, "mean_except_current", t // 2)
REF_SIZES = [(1, 1), (1, 255), (1, 257), (3, 173)]  # (npatch, len): 1, 255, 257, 519 complex values
REF_PAIRS = ["independent", "masked"]     # V independent of U; V = U * m, m in [0, 1]


def ref_inputs(t, npatch, length, pair, seed=0):
    """U, V (t, npatch, length, 2) fp32."""
    rng = np.random.default_rng(1000 * t + 10 * npatch + length + seed)
    u = rng.standard_normal((t, npatch, length, 2)).astype(F32)
    if pair == "independent":
        v = rng.standard_normal((t, npatch, length, 2)).astype(F32)
    else:
        v = u * rng.uniform(0, 1, size=(t, npatch, length, 1)).astype(F32)
    return u, v


def to_complex(a):
    a = np.asarray(a, dtype=np.float64)
    return (a[..., 0] + 1j * a[..., 1]).reshape(a.shape[0], -1)


def ref_sensitivity(Uc, Vc, bound):
    """Smallest, over every (f, o != f), of max_i |V_o[i] - U_o[i]| / ((t - 1) bound[f, i]) per component: by how many
    bounds the most sensitive element moves when one V_o is swapped for U_o (or back) in REF64[f]."""
    t = Uc.shape[0]
    d = np.stack([(Vc - Uc).real, (Vc - Uc).imag], axis=-1)
    worst = np.inf
    for f in range(t):
        for o in range(t):
            if o != f:
                worst = min(worst, float((np.abs(d[o]) / ((t - 1) * bound[f])).max()))
    return worst


# ------------------------------------------------------------------ B. smoothing and centring


def smooth64(x, window, subtract_mean):
    """(out, bound) of mc_field_smooth_center's contract on x (2, t, npatch), float64."""
    x = np.asarray(x, dtype=np.float64)
    t = x.shape[1]
    n = x.size
    big = float(np.abs(x).max())
    if window < 3:
        y = x.copy()
        bound = np.zeros_like(y)
    else:
        assert window <= t
        half = window // 2
        klo = -half if window & 1 else 1 - half
        y = np.empty_like(x)
        for i in range(half, t - half):
            y[:, i] = x[:, i + klo:i + half + 1].mean(axis=1)
        j = np.arange(window, dtype=np.float64)
        jm = 0.5 * (window - 1)
        for start, where in ((0, range(half)), (t - window, range(t - half, t))):
            seg = x[:, start:start + window]
            xm = seg.mean(axis=1)
            slope = ((j - jm)[None, :, None] * (seg - xm[:, None])).sum(axis=1) / ((j - jm) ** 2).sum()
            for i in where:
                y[:, i] = xm + slope * ((i - start) - jm)
        bound = U * np.abs(y) + 16 * window * EPS64 * big
    if subtract_mean:
        mean = y.mean()
        out = y - mean
        first = U * float(np.abs(y).mean()) if window >= 3 else 0.0  # the average of the first roundings
        bound = bound + first + U * (abs(mean) + np.abs(out)) + n * EPS64 * float(np.abs(y).max())
    else:
        out = y
    return out, bound * (1 + 8 * U)


SMOOTH_NPATCH = [1, 6, 127, 129, 300]
SMOOTH_T = [1, 2, 3, 4, 5, 9, 10, 40]
SAVGOL_T = [4, 6, 9, 10, 40]


def smooth_windows(t):
    return [0] + list(range(3, t + 1))


def smooth_field(t, npatch, kind):
    """(2, t, npatch) fp32.  'unit': N(0, 1), every series its own values (a wrong stride reads another series).
    'mean1000': N(1000, 1).  'grid1000': round(N(1000, 1)) + 0.75 * 2^-9 -- mean 1000, unit spread, and every value
    carries the same small fraction: once a thread's fp32 partial sum passes 2^15 that fraction is below half an ulp
    and is dropped by every addition, all in one direction, so a mean accumulated in fp32 is biased by far more than
    the bound (rounding errors of random fractions would cancel)."""
    rng = np.random.default_rng(7 * t + npatch)
    z = rng.standard_normal((2, t, npatch))
    if kind == "unit":
        return z.astype(F32)
    if kind == "mean1000":
        return (1000.0 + z).astype(F32)
    assert kind == "grid1000"
    return (np.round(1000.0 + z) + 0.75 * 2.0 ** -9).astype(F32)


def fp32_mean_by_threads(y, threads=256):
    """The mean of y (any shape, flattened in memory order) as 256 threads would form it with fp32 partial sums (thread
    i adds elements i, i + 256, ..) combined in double: the stand-in for a kernel that accumulates in fp32."""
    flat = np.asarray(y, dtype=F32).reshape(-1)
    pad = (-flat.size) % threads
    rows = np.concatenate([flat, np.zeros(pad, dtype=F32)]).reshape(-1, threads)
    acc = np.zeros(threads, dtype=F32)
    for r in rows:
        acc = (acc + r).astype(F32)
    return float(F32(acc.astype(np.float64).sum() / flat.size))


# ------------------------------------------------------------------ C. spline grids

M32 = {
    "bspline": ((1.0 / 6.0) * torch.tensor([[1, 4, 1, 0], [-3, 0, 3, 0], [3, -6, 3, 0], [-1, 3, -3, 1]],
                                           dtype=torch.float32)).double().numpy(),
    "catmull_rom": (0.5 * torch.tensor([[0, 2, 0, 0], [-1, 0, 1, 0], [2, -5, 4, -1], [-1, 3, -3, 1]],
                                       dtype=torch.float32)).double().numpy(),
}
GRID_TYPES = ["catmull_rom", "bspline"]


def knots32(n):
    return torch.linspace(0, 1, steps=max(n, 2))


def intervals(n, u):
    """(il, s64) of fp32 coordinates u on an axis of n samples: the fp32 knots and the fp32 coordinate decide the
    interval; s is the exact value of (u32 - knot32[il]) (n_eff - 1)."""
    u = torch.as_tensor(np.asarray(u, dtype=F32))
    pos = knots32(n)
    ne = pos.numel()
    il = torch.clamp(torch.searchsorted(pos, u.contiguous(), side="right") - 1, 0, ne - 2)
    s = (u.double() - pos.double()[il]) * float(ne - 1)
    return il.numpy(), s.numpy()


def _axis_tables(n, u, grid_type):
    """Dense per-axis operators for coordinates u (m,) on an axis of n samples (n_eff = max(n, 2) after duplication):
    P (m, n_eff + 2) the basis on the PADDED axis; W, E (m, n_eff) sum of |folded weight| and of its error bound per
    real sample."""
    M = M32[grid_type]
    il, s = intervals(n, u)
    ne = max(n, 2)
    m = len(il)
    p = np.stack([np.ones_like(s), s, s * s, s * s * s], axis=-1)
    b = p @ M
    e_b = (np.abs(p) * (np.array([0, 1, 3, 5]) + 4) * U) @ np.abs(M)
    P = np.zeros((m, ne + 2))
    rows = np.arange(m)
    for k in range(4):
        P[rows, il + k] += b[:, k]  # padded index of tap k: (il - 1 + k) + 1
    w, e = b.copy(), e_b.copy()
    lo = il == 0
    w[lo, 1] = b[lo, 1] + 2 * b[lo, 0]
    e[lo, 1] = e_b[lo, 1] + 2 * e_b[lo, 0] + U * np.abs(w[lo, 1])
    w[lo, 2] = b[lo, 2] - b[lo, 0]
    e[lo, 2] = e_b[lo, 2] + e_b[lo, 0] + U * np.abs(w[lo, 2])
    w[lo, 0] = e[lo, 0] = 0
    hi = il + 2 == ne
    w[hi, 2] = w[hi, 2] + 2 * b[hi, 3]
    e[hi, 2] = e[hi, 2] + 2 * e_b[hi, 3] + U * np.abs(w[hi, 2])
    w[hi, 1] = w[hi, 1] - b[hi, 3]
    e[hi, 1] = e[hi, 1] + e_b[hi, 3] + U * np.abs(w[hi, 1])
    w[hi, 3] = e[hi, 3] = 0
    W, E = np.zeros((m, ne)), np.zeros((m, ne))
    for k in range(4):
        idx = np.clip(il - 1 + k, 0, ne - 1)
        np.add.at(W, (rows, idx), np.abs(w[:, k]))
        np.add.at(E, (rows, idx), e[:, k])
    return P, W, E


def _pad(d, axis):
    first, second = np.take(d, [0], axis), np.take(d, [1], axis)
    last, penult = np.take(d, [-1], axis), np.take(d, [-2], axis)
    return np.concatenate([first - (second - first), d, last + (last - penult)], axis=axis)


def _prepared(data):
    d = np.asarray(data, dtype=np.float64)
    for axis in (1, 2, 3):
        if d.shape[axis] == 1:
            d = np.concatenate([d, d], axis=axis)
    padded = d
    for axis in (1, 2, 3):
        padded = _pad(padded, axis)
    return d, padded


def spline_lattice64(data, ut, uy, ux, grid_type):
    """(value (c, NT, NY, NX), bound) of the (c, nt, nh, nw) grid on the tensor-product lattice."""
    _, nt, nh, nw = np.shape(data)
    d, padded = _prepared(data)
    (Pt, Wt, Et), (Py, Wy, Ey), (Px, Wx, Ex) = (_axis_tables(n, u, grid_type) for n, u in ((nt, ut), (nh, uy), (nw, ux)))
    ein = lambda a, b, c, z: np.einsum("ia,jb,kc,zabc->zijk", a, b, c, z, optimize=True)  # noqa: E731
    val = ein(Pt, Py, Px, padded)
    ad = np.abs(d)
    bound = ein(Et, Wy, Wx, ad) + ein(Wt, Ey, Wx, ad) + ein(Wt, Wy, Ex, ad) + gamma(12) * ein(Wt, Wy, Wx, ad)
    return val, bound * (1 + 100 * U)


def spline_points64(data, tyx, grid_type):
    """(value (n, c), bound) of the grid at (n, 3) points."""
    _, nt, nh, nw = np.shape(data)
    d, padded = _prepared(data)
    tyx = np.asarray(tyx, dtype=F32).reshape(-1, 3)
    (Pt, Wt, Et), (Py, Wy, Ey), (Px, Wx, Ex) = (_axis_tables(n, tyx[:, a], grid_type) for a, n in enumerate((nt, nh, nw)))
    ein = lambda a, b, c, z: np.einsum("pa,pb,pc,zabc->pz", a, b, c, z, optimize=True)  # noqa: E731
    val = ein(Pt, Py, Px, padded)
    ad = np.abs(d)
    bound = ein(Et, Wy, Wx, ad) + ein(Wt, Ey, Wx, ad) + ein(Wt, Wy, Ex, ad) + gamma(12) * ein(Wt, Wy, Wx, ad)
    return val, bound * (1 + 100 * U)


SPLINE_GRIDS = [(2, 1, 1, 1), (2, 5, 1, 1), (2, 1, 3, 3), (2, 2, 2, 2), (2, 3, 2, 5), (1, 4, 3, 5), (3, 7, 6, 9),
                (2, 40, 5, 7)]
SPLINE_QUERIES = ["edge", "lin33", "mixed", "dense"]
POINT_COUNTS = [1, 255, 257, 1000]


def spline_grid(shape):
    rng = np.random.default_rng(sum(s * 31 ** i for i, s in enumerate(shape)))
    return (rng.standard_normal(shape) * 3.0 + 0.5).astype(F32)


def edge_vector(n):
    """The coordinates an interval search can get wrong on an axis of n samples: every knot, 0 and 1, the fp32
    neighbour below 1, an interior knot (n >= 3) and its two fp32 neighbours."""
    pos = knots32(n).numpy()
    u = [pos, np.array([0.0, 1.0, np.nextafter(F32(1), F32(0))], dtype=F32)]
    if len(pos) >= 3:
        k = pos[len(pos) // 2]
        u.append(np.array([np.nextafter(k, F32(0)), k, np.nextafter(k, F32(1))], dtype=F32))
    return np.concatenate(u).astype(F32)


def lin(n):
    return torch.linspace(0, 1, steps=n).numpy()


def spline_query(shape, kind):
    """(ut, uy, ux) fp32 coordinate vectors of one lattice case."""
    _, nt, nh, nw = shape
    if kind == "edge":
        return edge_vector(nt), edge_vector(nh), edge_vector(nw)
    if kind == "lin33":
        return lin(33), lin(33), lin(33)
    if kind == "mixed":
        return lin(1), lin(2), lin(33)
    assert kind == "dense"  # the field warp's lattice: the frame times and 10 points per control sample
    return lin(nt), lin(10 * nh), lin(10 * nw)


def spline_points(shape, n):
    """(n, 3) fp32 points: the eight corners of the cube first (n >= 8), then alternately uniform points and points
    whose coordinates come from the axes' edge vectors; n = 1: the corner (1, 1, 1)."""
    _, nt, nh, nw = shape
    rng = np.random.default_rng(n + nt + 10 * nh + 100 * nw)
    pts = rng.uniform(0, 1, size=(n, 3)).astype(F32)
    for a, size in enumerate((nt, nh, nw)):
        ev = edge_vector(size)
        pts[1::2, a] = ev[rng.integers(0, len(ev), size=len(pts[1::2]))]
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=F32)
    if n >= 8:
        pts[:8] = corners
    else:
        pts[:] = 1.0
    return pts


@functools.lru_cache(maxsize=None)
def lattice_case(shape, kind, grid_type):
    data = spline_grid(shape)
    q = spline_query(shape, kind)
    return (data, q) + spline_lattice64(data, *q, grid_type)


@functools.lru_cache(maxsize=None)
def points_case(shape, n, grid_type):
    data = spline_grid(shape)
    pts = spline_points(shape, n)
    return (data, pts) + spline_points64(data, pts, grid_type)


# ------------------------------------------------------------------ D. plan tables

MASK_CASES = [(63, 63, 15.75, 7.875), (48, 80, 12, 6), (33, 72, 8.25, 4.125), (100, 120, 25, 12.5),
              (121, 135, 30.25, 15.125), (64, 300, 16, 8), (130, 66, 16.5, 8.25),
              (32, 48, 12, 12), (32, 96, 24, 24),  # the local-motion convention: ring clipped; disk clipped in y
              (40, 24, 16, 4),                     # both x clamps
              (16, 16, 0.5, 3),                    # a one-pixel disk
              (33, 47, 9.5, 0),                    # no soft edge on an odd shape
              (24, 40, 0, 5)]                      # no disk at all: zeros


@functools.lru_cache(maxsize=None)
def mask64(h, w, radius, smoothing):
    """-> (inside bool, ring bool, value float64 (h, w), halfwidth per row: the largest a with (y, cx + a) inside,
    unclamped, -1 for an empty row).  All other pixels are 0."""
    r32, s32 = F32(radius), F32(smoothing)
    dy = (np.arange(h) - h // 2).astype(F32)[:, None]
    dx = (np.arange(w) - w // 2).astype(F32)[None, :]
    inside = np.sqrt((dy * dy + dx * dx).astype(F32)).astype(F32) < r32
    value = inside.astype(np.float64)
    ring = np.zeros_like(inside)
    if s32 > 0 and inside.any():
        d = ndimage.distance_transform_edt(~inside).astype(F32)
        ring = (d > 0) & (d <= s32)
        value[ring] = np.cos(np.pi / 2 * (d[ring].astype(np.float64) / float(s32)))
    a = np.arange(0, w + 1, dtype=F32)[None, :]
    row_in = np.sqrt((dy * dy + a * a).astype(F32)).astype(F32) < r32  # (h, w + 1): (y, cx + a) for a = 0 .. w
    halfw = np.where(row_in[:, 0], np.argmin(np.concatenate([row_in, np.zeros((h, 1), bool)], axis=1), axis=1) - 1, -1)
    return inside, ring, value, halfw


MASK_RING_BOUND = 6 * U

# (H, W, pixel spacing, B, (cuton, cutoff) in Angstrom, what it is there for)
FILTER_CASES = [(63, 64, 1.0, 500.0, (300.0, 10.0), "odd H"),
                (121, 135, 0.83, 500.0, (300.0, 10.0), "odd H and W, ps 0.83"),
                (48, 80, 1.5, 500.0, (300.0, 10.0), "H != W, ps 1.5"),
                (100, 120, 0.83, 500.0, (300.0, 3.0), "H != W, wide band"),
                (63, 48, 1.5, 0.0, (300.0, 10.0), "B = 0, odd H"),
                (64, 64, 1.0, 500.0, (8.0, 4.0), "band edges on bins"),
                (32, 32, 1.0, 500.0, (300.0, 2.0), "kyn = 0"),
                # high = 0.5 keeps row (H - 1) / 2 of an odd H, the one row whose sign the rule `ky < (H + 1) / 2` decides
                (63, 64, 1.0, 500.0, (300.0, 2.0), "odd H, every row kept")]


def kept_ky(H, kyp, kyn):
    return np.concatenate([np.arange(kyp), np.arange(H - kyn, H)]).astype(np.int64)


def filter64(W, H, nkx, kyp, kyn, low, high, B, ps):
    """-> (kept bool, value float64, bound, all (nkx, nky)) on the pruned grid filt[kx][kyi]."""
    ky = kept_ky(H, kyp, kyn)
    kk = np.where(ky < (H + 1) // 2, ky, ky - H)
    kx = np.arange(nkx)
    fy = (kk.astype(F32) * F32(1.0 / H)).astype(F32)[None, :]
    fx = (kx.astype(F32) * F32(1.0 / W)).astype(F32)[:, None]
    f = np.sqrt(((fy * fy).astype(F32) + (fx * fx).astype(F32)).astype(F32)).astype(F32)
    kept = (f > F32(low)) & (f <= F32(high))
    F = np.sqrt((kk[None, :] / H) ** 2 + (kx[:, None] / W) ** 2)
    expo = float(F32(B)) * (F / float(F32(ps))) ** 2 / 4
    value = np.where(kept, np.exp(-expo), 0.0)
    return kept, value, (12 * np.abs(expo) + 2) * U * value
