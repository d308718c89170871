"""float64 definitions, derived bounds, shared cases and comparisons for the conditioning and hot-pixel kernels
(csrc/condition.hip: mc_condition_movie, mc_raw_movie_stats; csrc/hot_pixels.hip: mc_condition_movie_hot,
mc_raw_hot_detect, mc_raw_hot_finalize, mc_hot_scatter_add; and with the engine each corrects, csrc/xc_rows_fwd.hip:
mc_xc_rows_hot_correct, csrc/warp_rigid_raw.hip: mc_warp_rigid_hot_taps, csrc/full_sums.hip: mc_full_rows_hot_correct).  tests/test_hot_reference_host.py checks this file on the host (independent restatements,
an fp32 stand-in that follows the kernels' operation order, deliberately wrong stand-ins that every comparison must
reject); tests/test_hot_kernels_float64.py runs the same comparisons on the kernels' output.

Definitions (numpy float64; x = float64(raw) * float64(gain) is the exact product of two fp32 values):

  condition64       x minus the float64 frame mean.
  hot64             per frame the population mean m and std sd, the limits m -+ thr sd, the hot set {x > hi or x < lo},
                    each hot pixel's replacement = mean of the up to 8 neighbours that are not hot, taken before any
                    replacement, the frame mean m if all are hot (the rule in the comment above cond_stats2_kernel), the
                    replaced frames, their means and the counts.
  undecided         the pixels within `delta` of a limit (below).  Every input of the tests has none: a condition on the
                    inputs, asserted on the host, not a tolerance.  With it the hot set of the fp32 kernels is the
                    float64 hot set and the complete list is compared entry for entry.
  stats64           raw_stats_finalize's definition: mu_f = mean of the (replaced) frame, the joint mean and unbiased
                    1 / std of the central box of x - mu_f over all frames, sub_f = mu_f + mean.
  rows_correction64 dT1[f - frame0, kx, y - y0] = sum (r - v) rstd mask[y, x] exp(-2 pi i kx x / W) over the entries of
                    frames [frame0, frame0 + njobs) and rows [y0, y0 + ny); the full-spectrum twin without mask and rstd
                    for kx = 0 .. W/2 and every row.
  warp_correction64 every output p of frame f gains (r - v) sum_k [clip(py + Sy - 1 + k) = qy] Wy[f, py, k]
                    sum_k [clip(px + Sx - 1 + k) = qx] Wx[f, k, px], evaluated for ALL outputs of the frame.
  scatter64         out[key] += val for 0 <= key < limit.

Bounds, u = 2^-24 (half an ulp, relative).  None is fitted to a kernel's output; each is a sum of named terms.

  frame mean  |mu32 - mean64| <= (A + P) u mean|x| + u |mean| + N 2^-53 mean|x|.  A: the fp32 roundings of a partial
              sum, each relative to sum|v| of that partial -- 3 for the depth-3 tree over 8 samples of the tiled kernels
              (cond_vec_kernel, raw_stats_kernel, raw_stats_hot_kernel), 15 sequential additions of cond_sum_kernel's
              16-sample partial, 0 where every sample is widened first (raw_stats_scalar_kernel, cond_stats2_kernel);
              P = 1 product rounding per sample (0 without a gain); u |mean| the final rounding to fp32; the last term
              the double accumulation of N samples (negligible, stated).
  sample      rigid_reference.conditioning_error (product and difference) + |mu32 - mean64|.
  delta       u |x| (the product) + u max|limit| (the limit's rounding to fp32) + dm + thr dsd, with
              dm = 4 u mean|x| (tree 3 + product 1), dq = 6 u mean(x^2) (the product twice through the square, the
              square's rounding, tree 3), dvar = dq + 2 |m| dm + dm^2, dsd = dvar / (2 sqrt(var - dvar)).
  list        keys, counts and the counter exact; v bit-equal to the numpy fp32 product; r within
              (n - 1) u sum|v_nb| / n (the n - 1 fp32 additions) + u |r| (the division) of the float64 mean of the fp32
              products of its n neighbours; with no neighbour left r = float32(m) of the kernel's own double sums, and m
              within dm of the float64 mean.  Against the float64 x the replacement carries u mean|x_nb| more.
  moments     sum v: (A + P) u sum|x|;  sum_box v: (B + P) u sum_box|x|;  sum_box v^2: (B + 2 P) u sum_box x^2, B = 8
              roundings of the sequential fused multiply-adds over a thread's 8 pixels (0 for the scalar kernel); after
              mc_raw_hot_finalize each adds the list terms in double, sum_hot e_r and sum_hot,box (2 |r| e_r + e_r^2);
              the first part stays relative to the UNREPLACED samples, over which the fp32 partials were formed (an
              int16 outlier of 30000 leaves 30000^2 u in its partial of sum_box v^2, which r^2 - v^2 cannot take back).
  mu, sub, mean_rstd   the moment bounds pushed through raw_stats_finalize's formulas to first order plus the squares
              of the first-order terms, and one rounding to fp32 each (stats_bounds, term by term).
  rows        per bin and component sum|dA| (sqrt2 1e-6 + 2 pi u + 3 u) + n_row u sum|dA| + u (|prefill| + sum|dA|):
              sqrt2 1e-6 is the figure mc_common.h states for these sine / cosine instructions, 2 pi u the rounding of
              ph / W, 3 u the roundings inside dA, one fp32 addition per entry of the row, and the last term the
              addition onto the pre-filled element, which a measurement of the CHANGE of T1 cannot avoid.
  records     out_key exact; val within (3 + (m_y - 1) + (m_x - 1)) u |r - v| sum|Wy| sum|Wx| over the m_y, m_x taps that
              clip onto the hot pixel (3 roundings of the product, up to 4 additions inside wy / wx at a clipped edge).
  scatter     a run of k equal keys within k u sum|val| + u |out before| (the k - 1 additions of the run and the
              addition onto out; the second term is that addition's rounding relative to the pre-filled value); entries
              without a key untouched bit for bit.
"""

from __future__ import annotations

import numpy as np

from kernel_harness import rng as _rng
from rigid_reference import KERNEL_SHIFT_POOL, conditioning_error

F32 = np.float32
U = 2.0 ** -24
HOT_NONE = (1 << 63) - 1
TRIG = np.sqrt(2.0) * 1e-6  # mc_common.h's figure for v_sin_f32 / v_cos_f32
KINDS = {"u8": (0, np.uint8), "i16": (1, np.int16), "f16": (2, np.float16), "f32": (3, np.float32)}
NB = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]  # hot_replacement's visiting order


# ------------------------------------------------------------------ definitions


def product64(raw, gain):
    x = np.asarray(raw).astype(np.float64)
    return x if gain is None else x * np.asarray(gain, dtype=np.float64)


def product32(raw, gain):
    """The kernels' sample: fp32(raw) * gain in fp32 (u8 / i16 / f16 widen exactly)."""
    x = np.asarray(raw).astype(F32)
    return x if gain is None else (x * np.asarray(gain, dtype=F32)).astype(F32)


def condition64(raw, gain, mean_zero):
    """-> (x - mean_f, mean_f), mean_f the float64 frame means (zeros without mean_zero)."""
    x = product64(raw, gain)
    mean = x.mean(axis=(1, 2)) if mean_zero else np.zeros(x.shape[0])
    return x - mean[:, None, None], mean


class Hot:
    """Result of hot64: m, sd, lo, hi (t,); hot (t, h, w) bool; keys (n,) ascending; r, v (n,) float64; nnb (n,) the
    number of neighbours averaged; nb_abs (n,) their sum|x|; replaced (t, h, w); mean_after, counts (t,)."""


def hot64(x, thr):
    x = np.asarray(x, dtype=np.float64)
    t, h, w = x.shape
    o = Hot()
    o.m, o.sd = x.mean(axis=(1, 2)), x.std(axis=(1, 2))
    o.lo, o.hi = o.m - thr * o.sd, o.m + thr * o.sd
    o.hot = (x > o.hi[:, None, None]) | (x < o.lo[:, None, None])
    o.replaced = x.copy()
    keys, r, v, nnb, nb_abs = [], [], [], [], []
    for f, y, xx in np.argwhere(o.hot):  # argwhere: ascending key order
        vals = [x[f, y + dy, xx + dx] for dy, dx in NB
                if 0 <= y + dy < h and 0 <= xx + dx < w and not o.hot[f, y + dy, xx + dx]]
        rep = float(np.mean(vals)) if vals else float(o.m[f])
        o.replaced[f, y, xx] = rep
        keys.append((int(f) * h + int(y)) * w + int(xx))
        r.append(rep)
        v.append(x[f, y, xx])
        nnb.append(len(vals))
        nb_abs.append(float(np.sum(np.abs(vals))) if vals else 0.0)
    o.keys = np.array(keys, dtype=np.int64)
    o.r, o.v = np.array(r, dtype=np.float64), np.array(v, dtype=np.float64)
    o.nnb, o.nb_abs = np.array(nnb, dtype=np.int64), np.array(nb_abs, dtype=np.float64)
    o.mean_after = o.replaced.mean(axis=(1, 2))
    o.counts = o.hot.sum(axis=(1, 2)).astype(np.int64)
    return o


def limit_error(x, thr):
    """(dm, dlimit) per frame: what the fp32 partial sums of 8 samples and the limit's rounding can move m and the
    limits by (the `delta` paragraph of the module docstring)."""
    x = np.asarray(x, dtype=np.float64)
    m, var = x.mean(axis=(1, 2)), x.var(axis=(1, 2))
    dm = 4 * U * np.abs(x).mean(axis=(1, 2))
    dq = 6 * U * (x * x).mean(axis=(1, 2))
    dvar = dq + 2 * np.abs(m) * dm + dm * dm
    assert (var > 4 * dvar).all(), "a frame without variance"
    dsd = dvar / (2 * np.sqrt(var - dvar))
    sd = np.sqrt(var)
    lim = np.maximum(np.abs(m - thr * sd), np.abs(m + thr * sd))
    return dm, dm + thr * dsd + U * lim


def undecided(x, thr):
    """(t, h, w) bool: the pixels whose side of a limit the fp32 kernels may decide differently from float64."""
    x = np.asarray(x, dtype=np.float64)
    m, sd = x.mean(axis=(1, 2)), x.std(axis=(1, 2))
    lo, hi = (m - thr * sd)[:, None, None], (m + thr * sd)[:, None, None]
    delta = U * np.abs(x) + limit_error(x, thr)[1][:, None, None]
    return (np.abs(x - lo) <= delta) | (np.abs(x - hi) <= delta)


def assert_decided(x, thr):
    """No undecided pixel at all -- hence none among the hot pixels' neighbours either (checked separately, as the
    condition is stated).  Returns hot64(x, thr)."""
    und = undecided(x, thr)
    assert not und.any(), f"{int(und.sum())} undecided pixels: choose another input"
    o = hot64(x, thr)
    near = np.zeros_like(o.hot)
    t, h, w = o.hot.shape
    for dy, dx in NB:
        near[:, max(0, dy):h + min(0, dy), max(0, dx):w + min(0, dx)] |= \
            o.hot[:, max(0, -dy):h + min(0, -dy), max(0, -dx):w + min(0, -dx)]
    assert not (near & und).any()
    return o


def central_box(h, w):
    return int(0.25 * h), int(0.75 * h), int(0.25 * w), int(0.75 * w)


def moments64(x, box):
    """(t, 3) float64: sum x, sum_box x, sum_box x^2 per frame."""
    hl, hu, wl, wu = box
    b = x[:, hl:hu, wl:wu]
    return np.stack([x.sum(axis=(1, 2)), b.sum(axis=(1, 2)), (b * b).sum(axis=(1, 2))], axis=1)


def stats64(x, box, mean_zero):
    """-> dict(mu (t,), mean, rstd, sub (t,)) of the frames x (replaced already where hot pixels are removed)."""
    hl, hu, wl, wu = box
    mu = x.mean(axis=(1, 2)) if mean_zero else np.zeros(x.shape[0])
    c = (x - mu[:, None, None])[:, hl:hu, wl:wu]
    mean = float(c.mean())
    return dict(mu=mu, mean=mean, rstd=1.0 / float(c.std(ddof=1)), sub=mu + mean)


def moment_bounds(x, box, with_gain, adds_sum, adds_box, hot=None, e_r=None):
    """(t, 3) bounds of the three moments (the `moments` paragraph).  `hot` / `e_r`: the float64 list and the bound
    of each replacement against float64 x -- the moments after mc_raw_hot_finalize."""
    hl, hu, wl, wu = box
    p = 1 if with_gain else 0
    b = np.abs(x[:, hl:hu, wl:wu])
    n = x.shape[1] * x.shape[2]
    dbl = n * 2.0 ** -53  # the double accumulation of n samples
    out = np.stack([((adds_sum + p) * U + dbl) * np.abs(x).sum(axis=(1, 2)),
                    ((adds_box + p) * U + dbl) * b.sum(axis=(1, 2)),
                    ((adds_box + 2 * p) * U + dbl) * (b * b).sum(axis=(1, 2))], axis=1)
    if hot is not None:
        t, h, w = x.shape
        f = hot.keys // (h * w)
        y, xx = (hot.keys % (h * w)) // w, hot.keys % w
        inbox = (y >= hl) & (y < hu) & (xx >= wl) & (xx < wu)
        np.add.at(out[:, 0], f, e_r)
        np.add.at(out[:, 1], f[inbox], e_r[inbox])
        np.add.at(out[:, 2], f[inbox], (2 * np.abs(hot.r) * e_r + e_r * e_r)[inbox])
    return out


def mean_error(x, with_gain, adds, extra_sum=0.0):
    """|mu32 - mean64| per frame (the `frame mean` paragraph); `extra_sum`: a further bound of the frame's sum."""
    n = x.shape[1] * x.shape[2]
    p = 1 if with_gain else 0
    return ((adds + p) * U + n * 2.0 ** -53) * np.abs(x).mean(axis=(1, 2)) + extra_sum / n + U * np.abs(x.mean(axis=(1, 2)))


def stats_bounds(x, box, mean_zero, mb):
    """Bounds of mu (t,), mean, rstd and sub (t,) from the moment bounds `mb` (t, 3) of moment_bounds, through
    raw_stats_finalize:  mu = fp32(sum / N);  S = sum_f (sb - n mu);  Q = sum_f (qb - 2 mu sb + n mu^2);
    mean = S / (n t);  var = (Q - n t mean^2) / (n t - 1);  rstd = fp32(1 / sqrt(var))."""
    hl, hu, wl, wu = box
    t = x.shape[0]
    N, n = x.shape[1] * x.shape[2], (hu - hl) * (wu - wl)
    ref = stats64(x, box, mean_zero)
    e_mu = (mb[:, 0] / N + U * np.abs(ref["mu"])) if mean_zero else np.zeros(t)
    b = x[:, hl:hu, wl:wu]
    sb = b.sum(axis=(1, 2))
    dS = mb[:, 1] + n * e_mu  # per frame, of sb - n mu
    # qb - 2 mu sb + n mu^2: d/d mu = -2 (sb - n mu)
    dQ = mb[:, 2] + 2 * np.abs(ref["mu"]) * mb[:, 1] + 2 * e_mu * (np.abs(sb - n * ref["mu"]) + mb[:, 1]) + n * e_mu ** 2
    nt = n * t
    e_mean0 = dS.sum() / nt
    var = 1.0 / ref["rstd"] ** 2
    # var = (Q - S^2 / nt) / (nt - 1): d/dS = -2 mean
    dvar = (dQ.sum() + 2 * abs(ref["mean"]) * dS.sum() + dS.sum() ** 2 / nt) / (nt - 1)
    assert var > 4 * dvar
    e_rstd = 0.5 * dvar / (var - dvar) ** 1.5 + U * ref["rstd"] * (1 + 1e-6)
    e_mean = e_mean0 + U * abs(ref["mean"])
    e_sub = e_mu + e_mean + U * (np.abs(ref["sub"]) + e_mu + e_mean)
    return dict(mu=e_mu, mean=e_mean, rstd=e_rstd, sub=e_sub)


def rows_correction64(keys, rv, mask, rstd, h, w, nkx, y0, ny, frame0, njobs, prefill_abs=None):
    """-> (dT1 complex128 (njobs, nkx, ny), per-component bound (njobs, nkx, ny) float64, touched (njobs, ny) bool).
    `mask` (h, w) or None, `rstd` a float (1.0 for the full-spectrum twin, which also has mask None, nkx = w/2 + 1,
    y0 = 0, ny = h).  rv (n, 2) = {r, v}.  The bound is the `rows` paragraph without the pre-fill term when
    `prefill_abs` is None."""
    d = np.zeros((njobs, nkx, ny), dtype=np.complex128)
    mag = np.zeros((njobs, ny))
    cnt = np.zeros((njobs, ny), dtype=np.int64)
    kx = np.arange(nkx, dtype=np.float64)
    for key, (r, v) in zip(np.asarray(keys, dtype=np.int64).tolist(), np.asarray(rv, dtype=np.float64)):
        f, q = divmod(key, h * w)
        y, x = divmod(q, w)
        if not (frame0 <= f < frame0 + njobs and y0 <= y < y0 + ny):
            continue
        cnt[f - frame0, y - y0] += 1
        m = 1.0 if mask is None else float(mask[y, x])
        dA = (r - v) * rstd * m
        d[f - frame0, :, y - y0] += dA * np.exp(-2j * np.pi * ((kx * x) % w) / w)
        mag[f - frame0, y - y0] += abs(dA)
    bound = (mag * (TRIG + 2 * np.pi * U + 3 * U) + cnt * U * mag)[:, None, :] * np.ones((1, nkx, 1))
    if prefill_abs is not None:
        bound = bound + U * (prefill_abs + mag[:, None, :])
    return d, bound, cnt > 0


def warp_correction64(keys, rv, Wy, Wx, S, h, w):
    """-> (correction (t, h, w) float64, bound (t, h, w) of the sum of the kernel's records per output).  Wy (t, h, 5),
    Wx (t, 5, w), S (t, 2) int: the kernel's own tables.  Evaluated over every output of the frame."""
    t = Wy.shape[0]
    out = np.zeros((t, h, w))
    bound = np.zeros((t, h, w))
    Wy, Wx = np.asarray(Wy, dtype=np.float64), np.asarray(Wx, dtype=np.float64)
    py, px = np.arange(h), np.arange(w)
    for key, (r, v) in zip(np.asarray(keys, dtype=np.int64).tolist(), np.asarray(rv, dtype=np.float64)):
        f, q = divmod(key, h * w)
        qy, qx = divmod(q, w)
        wy, ay, my = np.zeros(h), np.zeros(h), np.zeros(h)
        wx, ax, mx = np.zeros(w), np.zeros(w), np.zeros(w)
        for k in range(5):
            hit = np.clip(py + int(S[f, 0]) - 1 + k, 0, h - 1) == qy
            wy += hit * Wy[f, :, k]
            ay += hit * np.abs(Wy[f, :, k])
            my += hit
            hit = np.clip(px + int(S[f, 1]) - 1 + k, 0, w - 1) == qx
            wx += hit * Wx[f, k, :]
            ax += hit * np.abs(Wx[f, k, :])
            mx += hit
        out[f] += (r - v) * np.outer(wy, wx)
        adds = 3 + np.maximum(my - 1, 0)[:, None] + np.maximum(mx - 1, 0)[None, :]
        bound[f] += adds * U * abs(r - v) * np.outer(ay, ax)
    return out, bound


def scatter64(keys, vals, limit, out):
    """-> (out + scattered values, bound, touched) over the flat float64 copy of `out`."""
    res = np.asarray(out, dtype=np.float64).copy()
    mag, cnt = np.zeros_like(res), np.zeros(res.shape, dtype=np.int64)
    for k, v in zip(np.asarray(keys, dtype=np.int64).tolist(), np.asarray(vals, dtype=np.float64).tolist()):
        if 0 <= k < limit:
            res[k] += v
            mag[k] += abs(v)
            cnt[k] += 1
    return res, cnt * U * mag + U * np.abs(np.asarray(out, dtype=np.float64)) * (cnt > 0), cnt > 0


# ------------------------------------------------------------------ comparisons (host stand-ins and kernels alike)


def _ratio(d, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nan_to_num(np.asarray(d) / np.asarray(bound), nan=0.0, posinf=0.0).max(initial=0.0))


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound everywhere (NaN fails) -> worst ratio."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), got.shape)
    d = np.abs(got - ref)
    ok = d <= bound
    if not bool(np.all(ok)):
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} values beyond the bound, first at {tuple(int(v) for v in i)}: "
                             f"got {got[i]!r} ref {ref[i]!r} bound {bound[i]!r}")
    return _ratio(d, bound)


def check_condition(out, raw, gain, mean_zero, adds, what):
    """mc_condition_movie's output at every pixel against condition64."""
    ref, mean = condition64(raw, gain, mean_zero)
    x = product64(raw, gain)
    e_mu = mean_error(x, gain is not None, adds) if mean_zero else np.zeros(x.shape[0])
    bound = conditioning_error(raw, gain, mean) + e_mu[:, None, None]
    return assert_within(out, ref, bound, what)


def replacement_bound(h32):
    """Bound of an fp32 replacement against hot64 of the fp32 products (the `list` paragraph), all-hot entries 0."""
    n = np.maximum(h32.nnb, 1)
    return np.where(h32.nnb > 0, (n - 1) * U * h32.nb_abs / n + U * np.abs(h32.r), 0.0)


def check_list(keys, rv, counts, counter, raw, gain, thr, m_kernel, what, capacity=None):
    """The kernels' hot list (unsorted as written, or sorted) against hot64: keys and counts exact, v bit-equal,
    r within its bound; `m_kernel` (t,) the kernel's own frame means in double (hstats[:, 0] / N).  With `capacity`
    below the count only the written slots are compared, each a valid entry.  -> (worst ratio, hot64 of x)."""
    x = product64(raw, gain)
    v32 = product32(raw, gain)
    ref, h32 = hot64(x, thr), hot64(v32.astype(np.float64), thr)
    assert np.array_equal(ref.keys, h32.keys), f"{what}: the input has undecided pixels"
    keys, rv = np.asarray(keys, dtype=np.int64), np.asarray(rv)
    assert int(counter) == len(ref.keys), f"{what}: counter {int(counter)}, {len(ref.keys)} hot pixels"
    assert np.array_equal(np.asarray(counts, dtype=np.int64), ref.counts), f"{what}: counts {counts} != {ref.counts}"
    n = len(ref.keys) if capacity is None else min(capacity, len(ref.keys))
    assert len(keys) == n and rv.shape == (n, 2) and rv.dtype == F32, what
    order = np.argsort(keys, kind="stable")
    keys, rv = keys[order], rv[order]
    assert len(np.unique(keys)) == n, f"{what}: a key twice"
    pos = np.searchsorted(ref.keys, keys)
    assert (pos < len(ref.keys)).all() and np.array_equal(ref.keys[np.minimum(pos, len(ref.keys) - 1)], keys), \
        f"{what}: keys that are not hot pixels: {sorted(set(keys.tolist()) - set(ref.keys.tolist()))[:8]}, " \
        f"missing {sorted(set(ref.keys.tolist()) - set(keys.tolist()))[:8]}"
    assert np.array_equal(rv[:, 1], v32.reshape(-1)[keys]), f"{what}: v is not the fp32 product"
    allhot = h32.nnb[pos] == 0
    t, h, w = x.shape
    f = keys // (h * w)
    m_kernel = np.asarray(m_kernel, dtype=np.float64)
    assert np.array_equal(rv[allhot, 0], m_kernel[f[allhot]].astype(F32)), f"{what}: all-hot replacement is not fp32(m)"
    assert_within(m_kernel, ref.m, limit_error(x, thr)[0], f"{what} m")
    return assert_within(rv[:, 0], h32.r[pos], np.where(allhot, np.inf, replacement_bound(h32)[pos]), f"{what} r"), ref


def replacement_error64(ref, x, thr):
    """Bound of an fp32 replacement against the float64 list `ref` of x: replacement_bound + the products' roundings;
    an all-hot entry fp32(m): dm + u |m|."""
    t, h, w = x.shape
    f = ref.keys // (h * w)
    n = np.maximum(ref.nnb, 1)
    dm = limit_error(x, thr)[0]
    return np.where(ref.nnb > 0, (n * U * ref.nb_abs / n + U * np.abs(ref.r)) * (1 + 2 * U),
                    dm[f] + U * np.abs(ref.m[f]))


def check_condition_hot(out, raw, gain, mean_zero, thr, what):
    """mc_condition_movie_hot's output at every pixel: (hot ? r : x) - mean after replacement."""
    x = product64(raw, gain)
    ref = hot64(x, thr)
    t, h, w = x.shape
    e_r = replacement_error64(ref, x, thr)
    mean = ref.mean_after if mean_zero else np.zeros(t)
    e_mu = mean_error(ref.replaced, gain is not None, 0, np.bincount(ref.keys // (h * w), e_r, t)) if mean_zero \
        else np.zeros(t)
    bound = conditioning_error(raw, gain, mean) + e_mu[:, None, None]
    f = ref.keys // (h * w)
    bound.reshape(-1)[ref.keys] = e_r + U * (np.abs(ref.r) + np.abs(mean[f])) + e_mu[f]
    return assert_within(out, ref.replaced - mean[:, None, None], bound, what)


def check_rows(before, after, keys, rv, mask, rstd, h, w, nkx, y0, ny, frame0, njobs, what):
    """T1 (njobs, nkx, ny, 2) before / after mc_xc_rows_hot_correct: the change at every bin, rows no entry touches
    bit-equal."""
    before, after = np.asarray(before), np.asarray(after)
    d, bound, touched = rows_correction64(keys, rv, mask, rstd, h, w, nkx, y0, ny, frame0, njobs,
                                          np.abs(before.astype(np.float64)).max(axis=-1))
    same = np.broadcast_to(~touched[:, None, :, None], before.shape)
    assert np.array_equal(before[same], after[same]), f"{what}: a row without an entry changed"
    ch = after.astype(np.float64) - before.astype(np.float64)
    return max(assert_within(ch[..., 0], d.real, bound, f"{what} re"), assert_within(ch[..., 1], d.imag, bound, f"{what} im"))


def check_records(rec_key, rec_val, keys, rv, Wy, Wx, S, h, w, what):
    """mc_warp_rigid_hot_taps' 49 records per entry: the keys are exactly the outputs with a non-zero correction,
    no key twice within an entry, HOT_NONE records carry 0, the values summed per output within the bound."""
    rec_key, rec_val = np.asarray(rec_key, dtype=np.int64), np.asarray(rec_val, dtype=np.float64)
    n, t = len(keys), Wy.shape[0]
    assert rec_key.shape == (49 * n,) and rec_val.shape == (49 * n,), what
    ref, bound = warp_correction64(keys, rv, Wy, Wx, S, h, w)
    none = rec_key == HOT_NONE
    assert (rec_val[none] == 0).all(), f"{what}: a record without a key carries a value"
    k = rec_key[~none]
    assert ((k >= 0) & (k < t * h * w)).all(), f"{what}: key outside the movie"
    for e in range(n):
        ke = rec_key[49 * e:49 * e + 49]
        ke = ke[ke != HOT_NONE]
        assert len(np.unique(ke)) == len(ke), f"{what}: entry {e} writes an output twice"
        assert (ke // (h * w) == keys[e] // (h * w)).all(), f"{what}: entry {e} leaves its frame"
    got = np.zeros(t * h * w)
    np.add.at(got, k, rec_val[~none])
    got = got.reshape(t, h, w)
    # every output the definition reaches must carry a record (one output of several entries may cancel in `ref`,
    # so coverage is judged per entry by the bound: a missing record leaves |ref| > bound)
    return assert_within(got, ref, bound, what)


def check_scatter(before, after, keys, vals, limit, what):
    before, after = np.asarray(before), np.asarray(after)
    ref, bound, touched = scatter64(keys, vals, limit, before.reshape(-1))
    assert np.array_equal(before.reshape(-1)[~touched], after.reshape(-1)[~touched]), f"{what}: an element without a key changed"
    return assert_within(after.reshape(-1), ref, bound, what)


# ------------------------------------------------------------------ shared cases


def make_gain(h, w, seed=5):
    """fp32 gains in [0.8, 1.2], none equal to 1."""
    g = (0.8 + 0.4 * _rng(seed, h, w).random((h, w))).astype(F32)
    g[g == 1] = F32(1.01)
    return g


def make_raw(kind, t, h, w, seed=1):
    """Background of a raw movie: u8 counts that reach 255 and 0, i16 with negatives, f16 / f32 noise."""
    r = _rng(seed, t, h, w)
    if kind == "u8":
        raw = r.integers(0, 256, (t, h, w)).astype(np.uint8)
        raw.reshape(-1)[:2] = (255, 0)
        return raw
    if kind == "i16":
        return r.integers(-3000, 3001, (t, h, w)).astype(np.int16)
    x = r.normal(50.0, 20.0, (t, h, w))
    return x.astype(np.float16 if kind == "f16" else np.float32)


# (kind, (t, h, w), gain, mean_zero, raw offset in elements, out offset in floats); hw % 8 != 0 at (70, 90)
def condition_cases():
    cases = []
    for kind in KINDS:
        for shape in ((1, 70, 90), (9, 70, 90), (8, 64, 96), (9, 64, 96), (17, 64, 96)):
            cases.append((kind, shape, True, True, 0, 0))
        cases.append((kind, (9, 64, 96), False, True, 0, 0))   # the tiled kernel without a gain
        cases.append((kind, (9, 64, 96), True, True, 1, 0))    # base pointer off the 8 / 16-byte boundary
    cases += [("u8", (9, 70, 90), False, True, 0, 0), ("i16", (9, 64, 96), True, False, 0, 0),
              ("f32", (9, 64, 96), True, False, 0, 0), ("u8", (9, 70, 90), True, False, 0, 0),
              ("u8", (9, 64, 96), True, True, 0, 1), ("f32", (9, 64, 96), True, True, 0, 1),
              ("u8", (3, 64, 2056), True, True, 0, 0), ("i16", (3, 64, 2056), True, True, 0, 0),  # a partial workgroup
              ("u8", (2, 2056, 2048), True, True, 0, 0)]  # more than one grid sweep of 2048 x 256 x 8 pixels
    return cases


def condition_tiled(shape, raw_offset, out_offset):
    """mc_condition_movie's dispatch rule for buffers that are otherwise 16-byte aligned."""
    return (shape[1] * shape[2]) % 8 == 0 and raw_offset == 0 and out_offset == 0


# (kind, (t, h, w), box, mean_zero): tiled and scalar (w % 8 != 0), box edges inside and on an 8-pixel group
def stats_cases():
    out = []
    for kind in ("u8", "i16", "f32"):
        out += [(kind, (9, 64, 96), (16, 48, 24, 72), 1), (kind, (9, 64, 96), (10, 50, 19, 77), 1),
                (kind, (9, 70, 90), (17, 52, 22, 67), 1)]
    out += [("u8", (9, 64, 96), (10, 50, 19, 77), 0), ("i16", (9, 70, 90), (17, 52, 22, 67), 0)]
    return out


def hot_positions(h, w, kind):
    """((y, x) high outliers, (y, x) low outliers (i16 only)) planted in every frame: see the GPU cases of the module
    docstring of tests/test_hot_kernels_float64.py."""
    cy, cx = h // 2, w // 2
    hi = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1),                     # corners
          (0, w // 3), (h - 1, cx + 5), (h // 3, 0), (cy + 3, w - 1),         # first / last rows and columns
          (h // 4, 23), (h // 4, 40), (h // 4, 63),                           # 8k - 1, 8k, 8k + 7
          divmod(2047, w), divmod(2048, w),                                   # end / start of a workgroup's piece
          (cy, cx), (cy, cx + 1), (cy + 10, cx - 20), (cy + 11, cx - 20)]     # a horizontal and a vertical pair
    hi += [(cy - 15 + dy, cx + 9 + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]  # 3 x 3: the centre's neighbours all hot
    lo = [(cy - 9, cx + 21), (0, cx), (h - 2, 7), (cy - 9, cx + 22)] if kind == "i16" else []
    assert len(set(hi + lo)) == len(hi + lo)
    return hi, lo


# (kind, (t, h, w), thr)
HOT_CASES = [("u8", (3, 96, 128), 8.0), ("i16", (9, 96, 128), 8.0), ("i16", (3, 64, 2056), 8.0),
             ("u8", (9, 64, 2056), 8.0)]
WARP_CASES = [("u8", (6, 64, 128), 8.0), ("i16", (6, 64, 128), 8.0)]
P = KERNEL_SHIFT_POOL
# both signs, integer, half, |s| > 4; the last shift pushes most hot pixels' outputs under the zero-outside rule
WARP_SHIFTS = np.array([(P[0], P[1]), (P[3], P[4]), (P[4], P[5]), (P[6], P[7]), (P[9], P[8]), (40.5, -77.25)], dtype=F32)


def hot_movie(kind, shape, seed=3):
    """-> (raw, gain, planted (t, h, w) bool): a quiet background, the planted outliers of hot_positions in every frame
    and three more per frame at positions that move; gain non-trivial everywhere."""
    t, h, w = shape
    r = _rng(seed, t, h, w)
    if kind == "u8":
        raw = np.clip(np.rint(r.normal(24.0, 4.0, shape)), 1, 60).astype(np.uint8)
        top, bottom = 255, None
    else:
        raw = np.clip(np.rint(r.normal(200.0, 50.0, shape)), -100, 600).astype(np.int16)
        top, bottom = 30000, -30000
    planted = np.zeros(shape, dtype=bool)
    hi, lo = hot_positions(h, w, kind)
    for y, x in hi:
        raw[:, y, x] = top
        planted[:, y, x] = True
    for y, x in lo:
        raw[:, y, x] = bottom
        planted[:, y, x] = True
    for f in range(t):
        for j in range(3):
            y, x = h // 2 + 16 + 2 * (f % 5), 5 + 19 * j + 3 * f
            raw[f, y, x] = top
            planted[f, y, x] = True
    return raw, make_gain(h, w), planted


def rows_list(h, w, y0, ny, seed, single=False, skipped_first=True):
    """A hand-built sorted list for the row corrections over frames 0 .. 3 (the window is frame0 = 1, njobs = 2):
    several pixels of one row with x = 0 and x = w - 1, the same (y, x) in different frames, frames outside the window
    (the first entry in one), rows outside [y0, y0 + ny).  -> (keys (n,) int64, rv (n, 2) fp32, (ym, x0 mask, xf mask))."""
    r = _rng(seed, h, w)
    ym = y0 + ny // 2
    xz, xf = w // 2 - 3, w // 2 + 2  # mask exactly 0 / fractional there
    ent = set()
    if single:
        ent.add((1, ym, w // 3))
    else:
        rows_out = [y for y in (y0 - 1, y0 + ny) if 0 <= y < h]
        for f in (0, 1, 2, 3) if skipped_first else (1, 2, 3):
            for x in (0, 1, xz, xf, w // 2 + 7, w - 1):
                ent.add((f, ym, x))
            ent.add((f, y0, 5))
            ent.add((f, y0 + ny - 1, w - 2))
            for y in rows_out:
                ent.add((f, y, 9))
        ent.add((2, ym + 1, 0))
        ent.add((1, ym - 1, w - 1))
    keys = np.array(sorted((f * h + y) * w + x for f, y, x in ent), dtype=np.int64)
    rv = np.stack([r.normal(25, 3, len(keys)), r.normal(230, 30, len(keys))], axis=1).astype(F32)
    return keys, rv, (ym, xz, xf)


def rows_mask(h, w, ym, xz, xf, seed=2):
    m = np.ones((h, w), dtype=F32)
    m[:, :w // 4] = _rng(seed, h, w).random((h, w // 4)).astype(F32)
    m[ym, xz], m[ym, xf] = 0.0, 0.37
    return m


ROWS_SHAPES = ((64, 256), (96, 5760))   # power-of-two rows; one K3-format width
FULL_SHAPES = ((256, 64), (256, 5760))  # the smallest frames the row-major full-spectrum kernels take


def rows_geometry(h, w):
    """plan.xc_geometry with a mask small enough that rows lie outside its window [y0, y0 + ny), and a band that keeps a
    fraction of the columns."""
    from torch_motion_correction_amd import plan

    return plan.xc_geometry(h, w, 0.2, min(h, w) / 8, min(h, w) / 16)


def scatter_case(seed=4):
    """Hand-built sorted records for mc_hot_scatter_add over out[0, 1000): runs of 1, 2 and 300 equal keys, a run at
    i = 0, one across a 256-thread block boundary, one ending at m - 1, keys < 0, >= limit and HOT_NONE.
    -> (keys, vals, limit, out before)."""
    limit = 1000
    keys = [-7, -7, -1]                 # i = 0: a run without an output
    keys += [0, 0]                      # the first valid run, two entries
    keys += [3]                         # a single
    keys += [17] * 248                  # 6 .. 253
    keys += [40] * 6                    # 254 .. 259: crosses i = 256
    keys += [41]
    keys += [500] * 300                 # crosses two block boundaries
    keys += [999, 999, 999]
    keys += [1000, 1000, 123456]        # >= limit
    keys += [HOT_NONE] * 5
    keys = np.array(keys, dtype=np.int64)
    assert (np.diff(keys) >= 0).all()
    tail = np.array([2, 2, 998, 998], dtype=np.int64)
    r = _rng(seed)
    a = (keys, r.normal(0, 30, len(keys)).astype(F32))
    # a second list whose last run ends at m - 1 and whose first run starts at i = 0
    b = (tail, r.normal(0, 30, len(tail)).astype(F32))
    out = r.normal(0, 5, limit).astype(F32)
    return [a, b], limit, out
