"""Shared pieces of the rigid-warp tests (tests/test_rigid_shift_rounding_host.py, tests/test_rigid_routes.py,
tests/test_rigid_reference_host.py and tests/test_rigid_kernels_float64.py): the canonical per-frame pixel
shift, the cases the GPU tests run, and two float64 rigid resamplers that apply the reference's sampling rule to
an exact fp32 shift -- a dense one (matrices, frames of a few hundred pixels) and a gather-based one that is
usable at 4096 x 4096.

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


# ------------------------------------------------------------------ gather-based resampler (any frame size)


def cubic_weight_error(t):
    """Bound of |fp32 weight - float64 weight| for the four Keys weights of the fp32 fractions t (m,) -> (m, 4),
    absolute, for ATen's Horner forms evaluated in fp32 in any mix of separate and fused operations (fusing only
    removes roundings).  With u = 2^-24 and half-ulp roundings taken per binade of each intermediate:

      far taps, x = 1 + t or 2 - t in [1, 2]:  ((A x - 5A) x + 8A) x - 4A.  x itself is off by <= u and
        |p'| <= 0.75; A x in [-1.5, -0.75]: u; + 3.75 in [2.25, 3]: 2u (3u so far); * x in [3, 4.5]: 4u
        (3x + 4); - 6 in [-3, -1.5]: 2u (3x + 6); * x in [-3.1, -3]: 2u ((3x + 6) x + 2); + 3: the result,
        |w| <= 0.15, rounds by < 0.01u.  Sum: ((3x + 6) x + 3) u, 12u at x = 1 to 27u at x = 2.
      near taps, x = t or 1 - t in [0, 1]:  ((A + 2) x - (A + 3)) x x + 1.  1 - t is off by <= u/2 and |q'| <= 1.35;
        1.25 x: u; - 2.25: 2u (3u); * x, |.| <= 1.02: u (3x + 1); * x: u ((3x + 1) x + 1); + 1: u/2.
        Sum: ((3x + 1) x + 2.2) u, 2.2u to 6.2u.

    The error is ABSOLUTE: the far polynomial cancels from intermediates of magnitude 3 to 6 down to |w| <= 0.15
    (to ~2e-4 at a fraction of 2^-12), so it is not a number of ulps of the weight itself."""
    t = np.asarray(t, dtype=np.float64)

    def far(x):
        return (3 * x + 6) * x + 3

    def near(x):
        return (3 * x + 1) * x + 2.2

    return 2.0 ** -24 * np.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], axis=-1)


def axis_taps(n, s, weight_error=False):
    """One axis of n samples shifted by the fp32 shift s, per output index p: the four tap indices
    clip(floor(u) - 1 + k, 0, n - 1) (n, 4) int64, their float64 weights (n, 4) -- zero where the coordinate
    c = fp32(p + s) leaves [0, n - 1] -- and that inside mask (n,).  The rule of _axis_operator, tap by tap.
    `weight_error`: the weights are replaced by |w| + cubic_weight_error (zero outside as well)."""
    p = np.arange(n, dtype=F32)
    c = (p + F32(s)).astype(F32)
    inside = (c >= F32(0)) & (c <= F32(n - 1))
    u = _grid_chain(c, n)
    fl = np.floor(u)
    w = _cubic_weights((u - fl).astype(F32))
    if weight_error:
        w = np.abs(w) + cubic_weight_error((u - fl).astype(F32))
    w[~inside] = 0.0
    base = fl.astype(np.int64) - 1
    idx = np.clip(base[:, None] + np.arange(4)[None, :], 0, n - 1)  # border padding
    return idx, w, inside


def _gather_rows(f, idx, w, rows):
    """out[y] = sum_k w[y, k] f[idx[y, k]] for y in `rows` (the others stay zero)."""
    out = np.zeros((idx.shape[0],) + f.shape[1:], dtype=np.float64)
    if rows.size:
        acc = w[rows, 0, None] * f[idx[rows, 0]]
        for k in range(1, 4):
            acc += w[rows, k, None] * f[idx[rows, k]]
        out[rows] = acc
    return out


def rigid_resample_gather(frame, sy, sx, extra=(), weight_error=False):
    """rigid_resample by two separable passes of four gathers each: the same rule, the same return values
    (out, magnitude), for frames of any size.  The magnitude is sum_ij |wy_i| |wx_j| |v_ij| over the 16 taps as
    the kernels evaluate them: taps that clip to the same border sample are NOT merged before the absolute
    values are taken, so it is >= the dense resampler's |My| |f| |Mx|^T, with equality away from the border.
    `extra`: further non-negative (h, w) maps that are resampled with the absolute weights as well (an error map
    of the samples propagated to the output); their results follow the first two.  `weight_error`: one more map
    comes last, what the fp32 rounding of the cubic weights can move the output by:
    sum_ij ((|wy_i| + ey_i) (|wx_j| + ex_j) - |wy_i| |wx_j|) |v_ij| with e = cubic_weight_error."""
    f = np.asarray(frame, dtype=np.float64)
    h, w = f.shape
    iy, wy, in_y = axis_taps(h, sy)
    ix, wx, in_x = axis_taps(w, sx)
    rows, cols = np.flatnonzero(in_y), np.flatnonzero(in_x)

    def two_pass(src, a_y, a_x):
        tmp = _gather_rows(src, iy, a_y, rows)  # (h, w): the row pass
        if not rows.size or not cols.size:
            return np.zeros((h, w), dtype=np.float64)
        lo, hi = rows[0], rows[-1] + 1  # inside rows are contiguous: c is monotonic in p
        part = _gather_rows(np.ascontiguousarray(tmp[lo:hi].T), ix, a_x, cols)  # (w, hi - lo)
        out = np.zeros((h, w), dtype=np.float64)
        out[lo:hi] = part.T
        return out

    res = [two_pass(f, wy, wx), two_pass(np.abs(f), np.abs(wy), np.abs(wx))]
    res += [two_pass(np.asarray(e, dtype=np.float64), np.abs(wy), np.abs(wx)) for e in extra]
    if weight_error:
        ey, ex = axis_taps(h, sy, True)[1], axis_taps(w, sx, True)[1]
        res.append(two_pass(np.abs(f), ey, ex) - res[1])
    return tuple(res)


def rigid_resample_gather_stack(stack, shifts_px, extra=None, weight_error=False):
    """(t, h, w) stack and (t, 2) fp32 shifts -> (frames float64, magnitudes float64[, resampled extra maps]).
    `stack` may be a sequence of frames or a callable f -> frame, so that a large movie is widened to float64
    one frame at a time; `extra`, if given, is a callable f -> (h, w) error map of frame f."""
    sh = np.asarray(shifts_px, dtype=F32)
    get = stack if callable(stack) else (lambda f: stack[f])
    res = [rigid_resample_gather(get(f), sh[f, 0], sh[f, 1], () if extra is None else (extra(f),), weight_error)
           for f in range(sh.shape[0])]
    return tuple(np.stack(r) for r in zip(*res))


def condition_float64(raw, gain, mu):
    """The raw routes' conditioning in float64: v = float64(raw) * float64(gain) - float64(mu_f), `mu` the fp32
    per-frame means the kernels use (engine.RawMovie.mu read back; their accuracy is pinned by
    test_raw_movie_statistics_match_a_float64_reference).  raw (t, h, w) or (h, w) with a scalar mu."""
    raw = np.asarray(raw, dtype=np.float64)
    g = 1.0 if gain is None else np.asarray(gain, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    return raw * g - (mu[:, None, None] if raw.ndim == 3 else mu)


def conditioning_error(raw, gain, mu):
    """Per-sample bound of |fp32 conditioning - condition_float64|: c = raw * gain - mu in fp32 is at most two
    roundings (the product -- raw and gain are exact fp32 values -- and the difference, or one fused
    multiply-add), each at most 2^-24 of a magnitude <= |raw * gain| + |mu|: 2 * 2^-24 * (|raw * gain| + |mu|)."""
    raw = np.asarray(raw, dtype=np.float64)
    g = 1.0 if gain is None else np.asarray(gain, dtype=np.float64)
    mu = np.abs(np.asarray(mu, dtype=np.float64))
    return 2 * 2.0 ** -24 * (np.abs(raw * g) + (mu[:, None, None] if raw.ndim == 3 else mu))


def assert_frames(got, ref, bound, what, on_border=None):
    """Kernel frames (a torch tensor) against the float64 reference: the zero patterns are equal (no knife-edge
    mask; `on_border`, if given, marks the pixels whose zero rule is left to the kernel) and |got - ref| <= bound
    at every pixel.  Returns the worst |got - ref| / bound (0 / 0 counts as 0)."""
    got = got.detach().cpu().double().numpy()
    zr, zg = ref == 0, got == 0
    if on_border is not None:  # pixels where the zero rule is left to the kernel (see the caller)
        bound = np.where(on_border & (zr != zg), np.inf, bound)
        zg = np.where(on_border, zr, zg)
    if not np.array_equal(zr, zg):
        bad = np.argwhere(zr != zg)
        frames = sorted({int(f) for f in bad[:, 0]})
        rows = sorted({(int(f), int(y)) for f, y, _ in bad[:4096]})[:12]
        cols = sorted({(int(f), int(x)) for f, _, x in bad[:4096]})[:12]
        raise AssertionError(f"{what}: zero pattern differs in frames {frames}, (frame, row) {rows}, "
                             f"(frame, col) {cols}: {int((zr != zg).sum())} pixels")
    d = np.abs(got - ref)
    ok = d <= bound  # False for a NaN the kernel left or wrote
    if not bool(ok.all()):
        bad = np.argwhere(~ok)
        ratio = np.where(ok, 0.0, d / np.maximum(bound, 1e-300))
        worst = np.unravel_index(int(np.argmax(np.where(np.isnan(ratio), np.inf, ratio))), ratio.shape)
        raise AssertionError(f"{what}: {len(bad)} pixels beyond the bound, first (frame, row, col) "
                             f"{[tuple(int(v) for v in b) for b in bad[:8]]}, worst at {tuple(int(v) for v in worst)}: "
                             f"got {got[worst]!r} ref {ref[worst]!r} bound {bound[worst]!r}")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nan_to_num(d / bound, nan=0.0, posinf=0.0).max())


# ------------------------------------------------------------------ cases of tests/test_rigid_kernels_float64.py
# The shift values every kernel case cycles through, frame by frame and with the two axes out of step.  Per axis
# the values a kernel meets contain both signs, a fraction of exactly 0.5, a fraction below 2^-10, an integer and
# (x axis) integer parts floor(s) of every residue mod 4 -- the raw u8 kernel's sub-unit offset m takes all four,
# the i16 kernel's m and the fp16 kernel's window parity P both -- asserted by tests/test_rigid_reference_host.py.
KERNEL_SHIFT_POOL = (2.5, -7.0, 3.0 + 2.0 ** -12, -5.5, 4.0, -1.37, 9.61, -12.0 + 2.0 ** -11, 6.25, -3.5, 1.0,
                     -10.75)


def kernel_case_shifts(t, h, w, offset=0, n_pool=None, n_big=2):
    """(K, 2) fp32 shifts of one kernel case, K a multiple of t (the case runs K / t launches over the same
    frames): `n_pool` pairs from KERNEL_SHIFT_POOL (default: as few as make K a multiple of t), then
      - `n_big` shifts larger than a tile where the frame allows (beyond 32 rows for h >= 64, beyond 512 columns
        for w >= 1024; the window then lies wholly off its own tile and the border patch runs for interior tiles),
      - the shift that leaves one row and one column inside, (h - 1.5, -(w - 1.5)),
      - a shift >= n on one axis: an all-zero frame."""
    big = [(40.5 if h >= 64 else 10.5, -77.25), (-35.75 if h >= 64 else -(h - 6.75), 600.3 if w >= 1024 else 300.3)]
    extras = big[:n_big] + [(h - 1.5, -(w - 1.5))]
    extras.append((h + 0.5, 3.25) if offset % 2 == 0 else (-2.5, -(w + 3.0)))
    if n_pool is None:
        n_pool = next(n for n in range(1, t + 1) if (n + len(extras)) % t == 0)
    v = KERNEL_SHIFT_POOL
    pool = [(v[(offset + i) % len(v)], v[(offset + 3 * i + 1) % len(v)]) for i in range(n_pool)]
    sh = np.array(pool + extras, dtype=F32)
    assert sh.shape[0] % t == 0, (t, sh.shape)
    return sh


# kernel -> [(t, h, w, offset into the pool, n_pool, n_big)]
KERNEL_CASES = {
    "warp_rigid_dma": [(3, 33, 516, 0, 5, 2),    # last tile has one row and one quad
                       (3, 32, 512, 5, 2, 2),    # exactly one full tile
                       (4, 40, 1028, 7, 4, 2),
                       (3, 64, 2048, 2, 2, 2),   # 8 tiles: the XCD remap runs with full tiles
                       (3, 96, 1536, 9, 2, 2),   # 9 tiles: no remap
                       (3, 256, 4096, 4, 2, 2),
                       (2, 4096, 4096, 11, 1, 1)],  # benchmark geometry: 1024 tiles, remap on
    "warp_rigid": [(3, 130, 250, 0, 5, 2), (2, 96, 1030, 5, 4, 2), (3, 64, 512, 9, 5, 2)],
    "warp_rigid_dma_h": [(3, 33, 520, 0, 5, 2), (3, 64, 2048, 5, 5, 2), (2, 1024, 4096, 10, 1, 1),
                         (3, 40, 1032, 11, 2, 2)],
    "warp_rigid_raw": [(6, 33, 516, 0, 8, 2), (6, 64, 2048, 8, 8, 2), (4, 256, 4096, 4, 4, 2),
                       (2, 4096, 4096, 1, 1, 1)],  # the last one u8 only
}


def kernel_shift_coverage(values, x_axis, residues=4):
    """What a list of shift values along one axis lacks of the coverage above ([] = complete)."""
    v = np.asarray(values, dtype=F32).astype(np.float64)
    fr = v - np.floor(v)
    lack = []
    if not (v > 0).any() or not (v < 0).any():
        lack.append("both signs")
    if not (fr == 0.5).any():
        lack.append("a fraction of exactly 0.5")
    if not ((fr > 0) & (fr < 2.0 ** -10)).any():
        lack.append("a fraction below 2^-10")
    if not ((fr == 0) & (v != 0)).any():
        lack.append("a non-zero integer")
    if x_axis:
        have = {int(r) for r in np.floor(v).astype(np.int64) % residues}
        if have != set(range(residues)):
            lack.append(f"integer parts of every residue mod {residues}: {sorted(have)}")
    return lack


# Gain-cache re-centring of warp_rigid_raw (the cache holds RR_MY = RR_MX = 8 spare rows / columns around the
# first frame's window): the integer parts of consecutive frames' shifts jump by +5, +9, -9, -20, +20 in y, then
# by the same amounts in x, then on both axes at once, and return to the start.
RECENTRE_INTS = ((0, 0), (5, 0), (14, 0), (5, 0), (-15, 0), (5, 0),
                 (5, 5), (5, 14), (5, 5), (5, -15), (5, 5),
                 (14, 14), (-6, -6), (14, 14), (0, 0))
RECENTRE_SHIFTS = np.array([(a + 0.37, b + 0.81) for a, b in RECENTRE_INTS], dtype=F32)
