"""Host checks of tests/hot_reference.py (no GPU): the float64 definitions agree with independent naive restatements,
every input of tests/test_hot_kernels_float64.py has no undecided pixel, a numpy fp32 stand-in that follows the kernels'
operation order (csrc/condition.hip, csrc/hot_pixels.hip and the engines' correction kernels) lies inside every bound -- its worst error / bound is printed
and recorded in the GPU file's docstring -- and every comparison rejects a deliberately wrong stand-in."""

import numpy as np
import pytest

import hot_reference as hr
import rigid_reference as rr

F32, U = np.float32, hr.U


# ------------------------------------------------------------------ fp32 stand-ins (the kernels' operation order)


def tree8(v):
    """((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)) in fp32 over the last axis of length 8."""
    a = v[..., 0::2] + v[..., 1::2]
    b = a[..., 0::2] + a[..., 1::2]
    return b[..., 0] + b[..., 1]


def standin_frame_sums(v, tiled):
    """Per-frame sums of the fp32 samples v (t, h, w) as cond_vec_kernel (tree of 8, then double) or cond_sum_kernel
    (per thread, 16 sequential fp32 additions between flushes into a double) accumulate them."""
    t = v.shape[0]
    hw = v[0].size
    if tiled:
        return tree8(v.reshape(t, -1, 8)).astype(np.float64).sum(axis=1)
    stride = min(2048, (hw + 2047) // 2048) * 256
    nper = (hw + stride - 1) // stride
    out = np.zeros(t)
    for f in range(t):
        M = np.zeros(nper * stride, dtype=F32)
        M[:hw] = v[f].reshape(-1)
        M = M.reshape(nper, stride)
        s, ps = np.zeros(stride), np.zeros(stride, dtype=F32)
        for j in range(nper):
            ps = ps + M[j]
            if (j + 1) % 16 == 0:
                s, ps = s + ps, np.zeros(stride, dtype=F32)
        out[f] = (s + ps).sum()
    return out


def standin_condition(raw, gain, mean_zero, tiled):
    v = hr.product32(raw, gain)
    mean = (standin_frame_sums(v, tiled) / v[0].size).astype(F32) if mean_zero else np.zeros(v.shape[0], dtype=F32)
    return v - mean[:, None, None]


def standin_moments(raw, gain, box, tiled):
    """stats[f] = {sum v, sum_box v, sum_box v^2} as raw_stats_kernel / raw_stats_scalar_kernel form them."""
    v = hr.product32(raw, gain)
    t, h, w = v.shape
    hl, hu, wl, wu = box
    if not tiled:
        return hr.moments64(v.astype(np.float64), box)
    g = v.reshape(t, -1, 8)
    yy, xx = np.divmod(np.arange(h * w).reshape(-1, 8), w)
    bw = ((yy >= hl) & (yy < hu) & (xx >= wl) & (xx < wu)).astype(np.float64)
    ps, pq = np.zeros(g.shape[:2], dtype=F32), np.zeros(g.shape[:2], dtype=F32)
    for k in range(8):  # one rounding per fused multiply-add
        vk = g[..., k].astype(np.float64)
        ps = (ps.astype(np.float64) + bw[:, k] * vk).astype(F32)
        pq = (pq.astype(np.float64) + bw[:, k] * vk * vk).astype(F32)
    return np.stack([tree8(g).astype(np.float64).sum(axis=1), ps.astype(np.float64).sum(axis=1),
                     pq.astype(np.float64).sum(axis=1)], axis=1)


def standin_finalize(stats, N, n, mean_zero):
    """raw_stats_finalize."""
    t = stats.shape[0]
    mu = (stats[:, 0] / N).astype(F32) if mean_zero else np.zeros(t, dtype=F32)
    md = mu.astype(np.float64)
    S = (stats[:, 1] - n * md).sum()
    Q = (stats[:, 2] - 2 * md * stats[:, 1] + n * md * md).sum()
    NN = float(n * t)
    mean = S / NN
    var = max((Q - NN * mean * mean) / (NN - 1), 0.0)
    meanf = F32(mean)
    return dict(mu=mu, mean=meanf, rstd=F32(1.0 / np.sqrt(var)), sub=mu + meanf)


def standin_hot(raw, gain, thr, tiled_stats=True, wrong=None):
    """Detection and replacement as raw_stats_hot_kernel + raw_hot_detect_kernel (or cond_stats2_kernel +
    cond_hot_kernel with tiled_stats = False) -> dict(keys, rv, counts, m, out0, out1): the sorted list, the kernel's
    frame means in double, and mc_condition_movie_hot's output without / with mean_zero.
    wrong = 'gain': a neighbour's gain is read one element further; 'inplace': replacements read the frame as
    replaced so far."""
    v = hr.product32(raw, gain)
    t, h, w = v.shape
    N = h * w
    if tiled_stats:
        g = v.reshape(t, -1, 8)
        s = tree8(g).astype(np.float64).sum(axis=1)
        q = tree8(g * g).astype(np.float64).sum(axis=1)
    else:
        s, q = v.astype(np.float64).sum(axis=(1, 2)), (v.astype(np.float64) ** 2).sum(axis=(1, 2))
    m = s / N
    sd = np.sqrt(np.maximum(q / N - m * m, 0))
    lo, hi = (m - thr * sd).astype(F32), (m + thr * sd).astype(F32)
    hot = (v > hi[:, None, None]) | (v < lo[:, None, None])
    keys, rv = [], []
    cur = v.copy()
    rawf = np.asarray(raw).astype(F32)
    gflat = np.asarray(gain, dtype=F32).reshape(-1)
    for f, y, x in np.argwhere(hot):
        acc, n = F32(0), 0
        for dy, dx in hr.NB:
            yy, xx = y + dy, x + dx
            if not (0 <= yy < h and 0 <= xx < w):
                continue
            if wrong == "gain":
                val = F32(rawf[f, yy, xx] * gflat[(yy * w + xx + 1) % N])
            elif wrong == "inplace":
                val = cur[f, yy, xx]
            else:
                val = v[f, yy, xx]
            if val > hi[f] or val < lo[f]:
                continue
            acc = F32(acc + val)
            n += 1
        r = F32(acc / F32(n)) if n else F32(m[f])
        cur[f, y, x] = r
        keys.append((f * h + y) * w + x)
        rv.append((r, v[f, y, x]))
    keys, rv = np.array(keys, dtype=np.int64), np.array(rv, dtype=F32).reshape(-1, 2)
    rep = v.copy()
    rep.reshape(-1)[keys] = rv[:, 0]
    delta = np.bincount(keys // N, rv[:, 0].astype(np.float64) - rv[:, 1].astype(np.float64), t)
    mean_after = ((s + delta) / N).astype(F32)
    return dict(keys=keys, rv=rv, counts=hot.sum(axis=(1, 2)), m=m, s=s, out0=rep, out1=rep - mean_after[:, None, None])


def standin_hot_finalize(stats, hs, keys, rv, shape, box):
    """raw_hot_stats_fix on the moments `stats` (t, 3) with the detection sums hs (t,)."""
    t, h, w = shape
    hl, hu, wl, wu = box
    out = stats.copy()
    f, y, x = keys // (h * w), (keys % (h * w)) // w, keys % w
    r, v = rv[:, 0].astype(np.float64), rv[:, 1].astype(np.float64)
    inbox = (y >= hl) & (y < hu) & (x >= wl) & (x < wu)
    out[:, 0] = hs + np.bincount(f, r - v, t)
    out[:, 1] += np.bincount(f[inbox], (r - v)[inbox], t)
    out[:, 2] += np.bincount(f[inbox], (r * r - v * v)[inbox], t)
    return out


def standin_rows(T1, keys, rv, mask, rstd, h, w, nkx, y0, ny, frame0, njobs, wrong=None):
    """xc_rows_hot_fix / full_rows_hot_fix in fp32 (numpy's sine and cosine rounded to fp32).  wrong = 'conj': the
    phase conjugated; 'frame0': the window's first frame ignored."""
    out = T1.copy()
    kx = np.arange(nkx, dtype=np.int64)
    acc = {}
    for key, (r, v) in zip(keys.tolist(), rv):
        f, q = divmod(key, h * w)
        y, x = divmod(q, w)
        j = f if wrong == "frame0" else f - frame0
        if not (0 <= j < njobs and y0 <= y < y0 + ny):
            continue
        m = F32(1) if mask is None else mask[y, x]
        if m == 0:
            continue
        dA = F32(F32(F32(r - v) * F32(rstd)) * m)
        rev = ((kx * x) % w).astype(F32) / F32(w)
        c = np.cos(2 * np.pi * rev.astype(np.float64)).astype(F32)
        s = np.sin(2 * np.pi * rev.astype(np.float64)).astype(F32)
        ar, ai = acc.setdefault((j, y), [np.zeros(nkx, dtype=F32), np.zeros(nkx, dtype=F32)])
        acc[(j, y)] = [ar + dA * c, ai + dA * s if wrong == "conj" else ai - dA * s]
    for (j, y), (ar, ai) in acc.items():
        out[j, :, y - y0, 0] += ar
        out[j, :, y - y0, 1] += ai
    return out


def standin_taps(keys, rv, Wy, Wx, S, h, w, wrong=None):
    """warp_rigid_hot_taps in fp32.  wrong = 'clip': a tap that clips onto the hot pixel is dropped."""
    n = len(keys)
    rec_key = np.full(49 * n, hr.HOT_NONE, dtype=np.int64)
    rec_val = np.zeros(49 * n, dtype=F32)
    for e, key in enumerate(keys.tolist()):
        f, q = divmod(key, h * w)
        qy, qx = divmod(q, w)
        Sy, Sx = int(S[f, 0]), int(S[f, 1])
        for tap in range(49):
            py, px = qy - Sy - 4 + tap // 7, qx - Sx - 4 + tap % 7
            if not (0 <= py < h and 0 <= px < w):
                continue
            wy = wx = F32(0)
            for k in range(5):
                ry, rx = py + Sy - 1 + k, px + Sx - 1 + k
                if wrong != "clip":
                    ry, rx = min(max(ry, 0), h - 1), min(max(rx, 0), w - 1)
                if ry == qy:
                    wy = F32(wy + Wy[f, py, k])
                if rx == qx:
                    wx = F32(wx + Wx[f, k, px])
            if wy != 0 and wx != 0:
                rec_val[49 * e + tap] = F32(F32(F32(rv[e, 0] - rv[e, 1]) * wy) * wx)
                rec_key[49 * e + tap] = f * h * w + py * w + px
    return rec_key, rec_val


def standin_scatter(keys, vals, limit, out, wrong=None):
    """hot_scatter_add in fp32.  wrong = 'last': the last entry of a run is dropped."""
    res = out.copy()
    i, m = 0, len(keys)
    while i < m:
        j = i
        while j < m and keys[j] == keys[i]:
            j += 1
        if 0 <= keys[i] < limit:
            s = F32(0)
            for e in range(i, j - 1 if (wrong == "last" and j - i > 1) else j):
                s = F32(s + vals[e])
            res[keys[i]] = F32(res[keys[i]] + s)
        i = j
    return res


def rigid_tables(h, w, shifts):
    """Wy (t, h, 5), Wx (t, 5, w), S (t, 2) in the raw rigid warp's table layout, from rigid_reference's sampling rule:
    output p reads clip(p + S - 1 + k), k = 0 .. 4."""
    t = len(shifts)
    Wy, Wx, S = np.zeros((t, h, 5), dtype=F32), np.zeros((t, 5, w), dtype=F32), np.zeros((t, 2), dtype=np.int64)
    for f in range(t):
        for axis, n in ((0, h), (1, w)):
            s = F32(shifts[f, axis])
            p = np.arange(n, dtype=F32)
            c = (p + s).astype(F32)
            inside = (c >= 0) & (c <= F32(n - 1))
            u = rr._grid_chain(c, n)
            fl = np.floor(u)
            wt = rr._cubic_weights((u - fl).astype(F32))
            wt[~inside] = 0
            base = fl.astype(np.int64) - 1
            S[f, axis] = int((base - np.arange(n)).min()) + 1  # floor(s), or one less where the fp32 chain rounds down
            k0 = base - (np.arange(n) + S[f, axis] - 1)
            assert ((k0 >= 0) & (k0 <= 1)).all()
            for k in range(4):
                if axis == 0:
                    Wy[f, np.arange(n), k0 + k] = wt[:, k]
                else:
                    Wx[f, k0 + k, np.arange(n)] = wt[:, k]
    return Wy, Wx, S


# ------------------------------------------------------------------ the definitions against naive restatements


@pytest.mark.parametrize("shape", [(16, 32), (12, 30)])
@pytest.mark.parametrize("with_mask", [True, False])
def test_rows_correction_is_the_dft_of_the_deltas(shape, with_mask):
    h, w = shape
    y0, ny, nkx, frame0, njobs, rstd = 3, h - 6, w // 2 - 2, 1, 2, 0.21
    keys, rv, (ym, xz, xf) = hr.rows_list(h, w, y0, ny, 11)
    mask = hr.rows_mask(h, w, ym, xz, xf) if with_mask else None
    d, _, touched = hr.rows_correction64(keys, rv, mask, rstd, h, w, nkx, y0, ny, frame0, njobs)
    frames = np.zeros((4, h, w))
    for key, (r, v) in zip(keys.tolist(), rv.astype(np.float64)):
        f, q = divmod(key, h * w)
        frames[f, q // w, q % w] += (r - v) * rstd * (1.0 if mask is None else float(mask[q // w, q % w]))
    dense = np.fft.fft(frames, axis=-1)[frame0:frame0 + njobs, y0:y0 + ny, :nkx].transpose(0, 2, 1)
    assert np.abs(d - dense).max() <= 1e-11 * np.abs(dense).max()
    assert np.array_equal(touched, (frames[frame0:frame0 + njobs, y0:y0 + ny] != 0).any(axis=-1) |
                          (touched & (np.abs(dense).max(axis=1) == 0)))  # a mask-0 entry alone touches but adds 0
    assert touched.any() and not touched.all()


def test_warp_correction_is_the_difference_of_two_resamples():
    kind, shape, thr = hr.WARP_CASES[0]
    t, h, w = shape
    raw, gain, _ = hr.hot_movie(kind, shape)
    x = hr.product64(raw, gain)
    ref = hr.hot64(x, thr)
    Wy, Wx, S = rigid_tables(h, w, hr.WARP_SHIFTS)
    rv = np.stack([ref.r, ref.v], axis=1)
    corr, _ = hr.warp_correction64(ref.keys, rv, Wy, Wx, S, h, w)
    worst = 0.0
    for f in range(t):
        sy, sx = hr.WARP_SHIFTS[f]
        a = rr.rigid_resample_gather(ref.replaced[f], sy, sx)[0]
        b = rr.rigid_resample_gather(x[f], sy, sx)[0]
        scale = max(np.abs(a - b).max(), 1.0)
        worst = max(worst, np.abs(corr[f] - (a - b)).max() / scale)
    # the tables are fp32 roundings of the float64 weights: two weights per product
    assert worst <= 4 * U, worst
    assert (corr[5] == 0).mean() > 0.99 and np.abs(corr[:5]).max() > 10  # the zero-outside rule / real corrections


def test_scatter64_is_a_dictionary_sum():
    (lists, limit, out) = hr.scatter_case()
    keys, vals = lists[0]
    res, bound, touched = hr.scatter64(keys, vals, limit, out)
    want = out.astype(np.float64)
    for k in set(keys.tolist()):
        if 0 <= k < limit:
            want[k] += vals[keys == k].astype(np.float64).sum()
    assert np.allclose(res, want, rtol=0, atol=1e-9) and sorted(np.flatnonzero(touched)) == [0, 3, 17, 40, 41, 500, 999]
    runs = {int(k): int((keys == k).sum()) for k in np.flatnonzero(touched)}
    assert runs == {0: 2, 3: 1, 17: 248, 40: 6, 41: 1, 500: 300, 999: 3}
    first40 = int(np.flatnonzero(keys == 40)[0])
    assert first40 < 256 <= first40 + 5  # the run crosses a 256-thread block boundary


# ------------------------------------------------------------------ the inputs of the GPU tests


@pytest.mark.parametrize("case", hr.HOT_CASES + hr.WARP_CASES, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}")
def test_gpu_inputs_have_no_undecided_pixel(case):
    kind, shape, thr = case
    raw, gain, planted = hr.hot_movie(kind, shape)
    x = hr.product64(raw, gain)
    ref = hr.assert_decided(x, thr)
    assert np.array_equal(ref.hot, planted), "the hot set is not the planted set"
    assert (gain != 1).all()
    assert (ref.nnb == 0).sum() == shape[0], "one pixel per frame whose neighbours are all hot"
    und = int(hr.undecided(x, thr).sum())
    print(f"UNDECIDED {kind} {shape}: {und} pixels, {len(ref.keys)} hot")
    assert und == 0


# ------------------------------------------------------------------ the fp32 stand-in inside every bound


def _case_data(case):
    kind, shape, with_gain, mean_zero, roff, ooff = case
    t, h, w = shape
    return hr.make_raw(kind, t, h, w), (hr.make_gain(h, w) if with_gain else None)


@pytest.mark.parametrize("case", [c for c in hr.condition_cases() if c[1] != (2, 2056, 2048)],
                         ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-g{int(c[2])}-m{int(c[3])}-o{c[4]}{c[5]}")
def test_condition_standin_is_inside_the_bound(case):
    kind, shape, with_gain, mean_zero, roff, ooff = case
    raw, gain = _case_data(case)
    tiled = hr.condition_tiled(shape, roff, ooff)
    out = standin_condition(raw, gain, mean_zero, tiled)
    r = hr.check_condition(out, raw, gain, mean_zero, 3 if tiled else 15, str(case))
    print(f"RATIO standin condition {case}: {r:.3f}")
    if mean_zero:  # a mean that is off by 4e-6 of the frame's level is rejected
        with pytest.raises(AssertionError):
            hr.check_condition(out + F32(4e-6) * np.abs(out).max(), raw, gain, mean_zero, 3 if tiled else 15, "wrong")


@pytest.mark.parametrize("case", hr.stats_cases(), ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}-{c[2][2]}-m{c[3]}")
def test_stats_standin_is_inside_the_bound(case):
    kind, shape, box, mean_zero = case
    t, h, w = shape
    raw, gain = hr.make_raw(kind, t, h, w, 7), hr.make_gain(h, w)
    tiled = w % 8 == 0
    x = hr.product64(raw, gain)
    mom = standin_moments(raw, gain, box, tiled)
    mb = hr.moment_bounds(x, box, True, 3 if tiled else 0, 8 if tiled else 0)
    worst = hr.assert_within(mom, hr.moments64(x, box), mb, "moments")
    fin = standin_finalize(mom, h * w, (box[1] - box[0]) * (box[3] - box[2]), mean_zero)
    ref, sb = hr.stats64(x, box, mean_zero), hr.stats_bounds(x, box, mean_zero, mb)
    for k in ("mu", "mean", "rstd", "sub"):
        worst = max(worst, hr.assert_within(fin[k], ref[k], sb[k], k))
    print(f"RATIO standin stats {case}: {worst:.3f}")
    with pytest.raises(AssertionError):  # the box one column off
        wrong = standin_moments(raw, gain, (box[0], box[1], box[2] + 1, box[3] + 1), tiled)
        hr.assert_within(wrong, hr.moments64(x, box), mb, "moments")


@pytest.mark.parametrize("case", hr.HOT_CASES, ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}")
def test_hot_standin_is_inside_the_bound_and_wrong_ones_are_not(case):
    kind, shape, thr = case
    t, h, w = shape
    raw, gain, _ = hr.hot_movie(kind, shape)
    x = hr.product64(raw, gain)
    box = hr.central_box(h, w)
    s = standin_hot(raw, gain, thr)
    r_list, ref = hr.check_list(s["keys"], s["rv"], s["counts"], len(s["keys"]), raw, gain, thr, s["m"], "list")
    # mc_condition_movie_hot: every sample widened before it is summed
    c = standin_hot(raw, gain, thr, tiled_stats=False)
    r_out = max(hr.check_condition_hot(c["out1"], raw, gain, True, thr, "hot out"),
                hr.check_condition_hot(c["out0"], raw, gain, False, thr, "hot out, no mean"))
    # moments after mc_raw_hot_finalize, and what raw_stats_finalize makes of them
    e_r = hr.replacement_error64(ref, x, thr)
    mom = standin_hot_finalize(standin_moments(raw, gain, box, True), s["s"], s["keys"], s["rv"], shape, box)
    mb = hr.moment_bounds(x, box, True, 3, 8, ref, e_r)  # the sums were formed over the UNREPLACED samples
    r_st = hr.assert_within(mom, hr.moments64(ref.replaced, box), mb, "moments after finalize")
    for mean_zero in (1, 0):
        fin = standin_finalize(mom, h * w, (box[1] - box[0]) * (box[3] - box[2]), mean_zero)
        want, sb = hr.stats64(ref.replaced, box, mean_zero), hr.stats_bounds(ref.replaced, box, mean_zero, mb)
        for k in ("mu", "mean", "rstd", "sub"):
            r_st = max(r_st, hr.assert_within(fin[k], want[k], sb[k], k))
    print(f"RATIO standin hot {case}: list {r_list:.3f} output {r_out:.3f} moments {r_st:.3f}")
    # overflow: the first slots only
    hr.check_list(s["keys"][5:21], s["rv"][5:21], s["counts"], len(s["keys"]), raw, gain, thr, s["m"], "overflow", 16)
    for wrong in ("gain", "inplace"):
        bad = standin_hot(raw, gain, thr, wrong=wrong)
        with pytest.raises(AssertionError):
            hr.check_list(bad["keys"], bad["rv"], bad["counts"], len(bad["keys"]), raw, gain, thr, bad["m"], wrong)
        bad = standin_hot(raw, gain, thr, tiled_stats=False, wrong=wrong)
        with pytest.raises(AssertionError):
            hr.check_condition_hot(bad["out1"], raw, gain, True, thr, wrong)
    with pytest.raises(AssertionError):  # a list without its last entry
        hr.check_list(s["keys"][:-1], s["rv"][:-1], s["counts"], len(s["keys"]), raw, gain, thr, s["m"], "short")


def _rows_setup(h, w, full, variant):
    if full:
        nkx, y0, ny = w // 2 + 1, 0, h
    else:
        g = hr.rows_geometry(h, w)
        assert g.W == w and g.y0 + g.ny <= h
        nkx, y0, ny = g.nkx, g.y0, g.ny
    keys, rv, (ym, xz, xf) = hr.rows_list(h, w, y0, ny, 13, single=variant == "single",
                                          skipped_first=variant != "first-in-window")
    mask = hr.rows_mask(h, w, ym, xz, xf) if (variant != "nomask" and not full) else None
    return keys, rv, mask, nkx, y0, ny


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("variant", ["all", "nomask", "single", "first-in-window"])
def test_rows_standin_is_inside_the_bound_and_wrong_ones_are_not(full, variant):
    worst = 0.0
    for h, w in (hr.FULL_SHAPES if full else hr.ROWS_SHAPES):
        keys, rv, mask, nkx, y0, ny = _rows_setup(h, w, full, variant)
        rstd = 1.0 if full else 0.21
        if not full and variant == "all":
            assert 0 < y0 and y0 + ny < h, "rows outside the window exist"
            assert keys[0] < h * w  # the first entry belongs to a skipped frame
        T1 = hr._rng(5, h, w).normal(0, 3, (2, nkx, ny, 2)).astype(F32)
        args = (keys, rv, mask, rstd, h, w, nkx, y0, ny, 1, 2)
        worst = max(worst, hr.check_rows(T1, standin_rows(T1, *args), *args, f"rows {(h, w)} {variant}"))
        for wrong in ("conj", "frame0"):
            with pytest.raises(AssertionError):
                hr.check_rows(T1, standin_rows(T1, *args, wrong=wrong), *args, wrong)
    print(f"RATIO standin rows full={full} {variant}: {worst:.3f}")


@pytest.mark.parametrize("case", hr.WARP_CASES, ids=lambda c: c[0])
def test_records_standin_is_inside_the_bound_and_a_dropped_clipped_tap_is_not(case):
    kind, shape, thr = case
    t, h, w = shape
    raw, gain, _ = hr.hot_movie(kind, shape)
    s = standin_hot(raw, gain, thr)
    Wy, Wx, S = rigid_tables(h, w, hr.WARP_SHIFTS)
    args = (s["keys"], s["rv"], Wy, Wx, S, h, w)
    r = hr.check_records(*standin_taps(*args), *args, "records")
    print(f"RATIO standin records {case}: {r:.3f}")
    with pytest.raises(AssertionError):
        hr.check_records(*standin_taps(*args, wrong="clip"), *args, "clip")
    # the definition reaches no output outside the kernel's 7 x 7 window: every non-zero correction has a record
    ref, _ = hr.warp_correction64(*args)
    rk, _ = standin_taps(*args)
    covered = np.zeros(t * h * w, dtype=bool)
    covered[rk[rk != hr.HOT_NONE]] = True
    assert not ((ref.reshape(-1) != 0) & ~covered).any()


def test_scatter_standin_is_inside_the_bound_and_a_dropped_entry_is_not():
    lists, limit, out = hr.scatter_case()
    worst = 0.0
    for keys, vals in lists:
        worst = max(worst, hr.check_scatter(out, standin_scatter(keys, vals, limit, out), keys, vals, limit, "scatter"))
        with pytest.raises(AssertionError):
            hr.check_scatter(out, standin_scatter(keys, vals, limit, out, wrong="last"), keys, vals, limit, "last")
    print(f"RATIO standin scatter: {worst:.3f}")
