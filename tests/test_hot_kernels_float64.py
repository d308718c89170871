"""The conditioning, raw-statistics and hot-pixel kernels (csrc/condition.hip, csrc/hot_pixels.hip, and the corrections
that live with their engines: xc_rows_hot_fix of csrc/xc_rows_fwd.hip, warp_rigid_hot_taps of csrc/warp_rigid_raw.hip,
full_rows_hot_fix of csrc/full_sums.hip)
against the float64 definitions of tests/hot_reference.py, whose docstring derives every bound.  No pixel, list entry or
bin is skipped; every test asserts which entry points of libmcorr ran (a recorder around the loaded library).

Cases (shared with tests/test_hot_reference_host.py, which asserts that no input has an undecided pixel):

  mc_condition_movie   u8 / i16 / f16 / f32; the tiled kernel (hw % 8 == 0, aligned) and the per-frame kernels (hw % 8 != 0
                       at (70, 90), a raw view one element off the 8 / 16-byte boundary, a misaligned out); gain and None;
                       mean_zero on and off; nframes 1, 8, 9, 17 (a partial 8-frame tile, blockIdx.y > 0); (64, 2056): a
                       partial workgroup; u8 (2, 2056, 2048): more than one grid sweep.
  mc_raw_movie_stats   tiled and scalar (w % 8 != 0), box edges inside and on an 8-pixel group, nframes 9, mean_zero 0 / 1.
  hot pixels           mc_condition_movie_hot and mc_raw_hot_detect + mc_raw_hot_finalize on the same movies, (96, 128) and
                       (64, 2056), nframes 3 and 9, u8 and i16, a gain that is not 1 anywhere; outliers at the corners, on
                       the first / last rows and columns, at 8k - 1, 8k, 8k + 7 of a row, at pixel 2047 and 2048 of a frame,
                       as a horizontal and a vertical pair, as a 3 x 3 block (its centre takes the frame mean), low ones for
                       i16, the same positions in every frame and three that move; one list overflow.
  row corrections      mc_xc_rows_hot_correct at (64, 256) and (96, 5760), mc_full_rows_hot_correct at (256, 64) and
                       (256, 5760), hand-built lists into pre-filled T1 / S: rows_list's entries, mask with an exact 0 and a
                       fraction, mask None, n = 1, a first entry inside and outside the frame window.
  warp corrections     engine.RawMovie + engine.warp_rigid_raw, (6, 64, 128) u8 / i16, shifts of KERNEL_SHIFT_POOL and one
                       that zeroes most outputs; the records against warp_correction64 over ALL outputs; frames and sum
                       against the float64 rigid resample of the replaced movie with test_rigid_kernels_float64's bound
                       formed over the samples the kernel resampled (the unreplaced movie) plus the records' bound and the
                       addition: fp32 cannot take the hot sample's own rounding, 32 u |w| |v|, back with r - v.
                       mc_hot_scatter_add alone on scatter_case's runs.

Measured worst error / bound: the GPU column is outstanding (no MI355X run of this file has been recorded yet); the
fp32 CPU stand-in's ratios are from tests/test_hot_reference_host.py.

                                                  kernels    fp32 CPU stand-in
  mc_condition_movie                                         0.327
  mc_raw_movie_stats                                         0.481
  hot list r / conditioned output / moments                  0.579 / 0.500 / 0.119
  row corrections (xc / full)                                0.131 / 0.104
  warp records                                               0.654
  mc_hot_scatter_add                                         0.302
"""

import ctypes as C

import numpy as np
import pytest
import torch

import hot_reference as hr
from kernel_harness import calls, ratios_fixture, worse  # noqa: F401
from rigid_reference import (assert_frames, condition_float64, conditioning_error, rigid_resample_gather_stack)

pytestmark = pytest.mark.gpu

F32, U = np.float32, hr.U


def _api():
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    return check, ptr, stream_ptr


def _dev_view(a, dev, offset=0):
    """numpy array -> device tensor that starts `offset` elements past a 256-byte boundary."""
    src = torch.from_numpy(np.ascontiguousarray(a))
    flat = torch.zeros(src.numel() + 64, dtype=src.dtype, device=dev)
    assert flat.data_ptr() % 256 == 0
    view = flat[offset:offset + src.numel()].view(src.shape)
    view.copy_(src)
    return view


def _ids(c):
    return "-".join("x".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


ratios = ratios_fixture()


# ------------------------------------------------------------------ mc_condition_movie


@pytest.mark.parametrize("case", hr.condition_cases(), ids=_ids)
def test_condition_movie_matches_float64(calls, dev, ratios, case):
    check, ptr, stream_ptr = _api()
    kind, shape, with_gain, mean_zero, roff, ooff = case
    t, h, w = shape
    raw = hr.make_raw(kind, t, h, w)
    gain = hr.make_gain(h, w) if with_gain else None
    rd = _dev_view(raw, dev, roff)
    gd = None if gain is None else _dev_view(gain, dev)
    n = t * h * w
    guard = torch.full((n + 64,), float("nan"), dtype=torch.float32, device=dev)
    out = guard[32 + ooff:32 + ooff + n].view(t, h, w)
    tiled = hr.condition_tiled(shape, roff, ooff)
    esize = rd.element_size()
    assert tiled == ((h * w) % 8 == 0 and rd.data_ptr() % (8 if kind == "u8" else 16) == 0 and out.data_ptr() % 16 == 0)
    assert (rd.data_ptr() // esize) % (16 // esize) == roff and (out.data_ptr() // 4) % 4 == ooff
    sums = torch.full((t,), float("nan"), dtype=torch.float64, device=dev) if mean_zero else None
    check(calls.mc_condition_movie(ptr(rd), hr.KINDS[kind][0], ptr(gd), t, h * w, int(mean_zero), ptr(sums), ptr(out),
                                   stream_ptr(dev)), "mc_condition_movie")
    torch.cuda.synchronize()
    calls.ran("mc_condition_movie")
    g = guard.cpu().numpy()
    assert np.isnan(g[:32 + ooff]).all() and np.isnan(g[32 + ooff + n:]).all(), "wrote outside its output"
    r = hr.check_condition(out.cpu().numpy(), raw, gain, mean_zero, 3 if tiled else 15, _ids(case))
    print(f"RATIO mc_condition_movie {_ids(case)}: {r:.3f}")
    worse(ratios, "mc_condition_movie", r)


# ------------------------------------------------------------------ mc_raw_movie_stats


def _raw_stats(calls, dev, rd, kind, gd, shape, box, mean_zero):
    check, ptr, stream_ptr = _api()
    t, h, w = shape
    stats = torch.full((t, 3), float("nan"), dtype=torch.float64, device=dev)
    mu, sub = torch.empty(t, device=dev), torch.empty(t, device=dev)
    mean_rstd = torch.empty(2, device=dev)
    check(calls.mc_raw_movie_stats(ptr(rd), hr.KINDS[kind][0], ptr(gd), t, h, w, *box, mean_zero, ptr(stats), ptr(mu),
                                   ptr(sub), ptr(mean_rstd), stream_ptr(dev)), "mc_raw_movie_stats")
    torch.cuda.synchronize()
    return stats.cpu().numpy(), dict(mu=mu.cpu().numpy(), sub=sub.cpu().numpy(), mean=float(mean_rstd[0]),
                                     rstd=float(mean_rstd[1]))


def _check_stats(got, x, box, mean_zero, mb, what):
    ref, sb = hr.stats64(x, box, mean_zero), hr.stats_bounds(x, box, mean_zero, mb)
    return max(hr.assert_within(got[k], ref[k], sb[k], f"{what} {k}") for k in ("mu", "mean", "rstd", "sub"))


@pytest.mark.parametrize("case", hr.stats_cases(), ids=_ids)
def test_raw_movie_stats_match_float64(calls, dev, ratios, case):
    kind, shape, box, mean_zero = case
    t, h, w = shape
    raw, gain = hr.make_raw(kind, t, h, w, 7), hr.make_gain(h, w)
    tiled = w % 8 == 0
    stats, fin = _raw_stats(calls, dev, _dev_view(raw, dev), kind, _dev_view(gain, dev), shape, box, mean_zero)
    calls.ran("mc_raw_movie_stats")
    x = hr.product64(raw, gain)
    mb = hr.moment_bounds(x, box, True, 3 if tiled else 0, 8 if tiled else 0)
    r = max(hr.assert_within(stats, hr.moments64(x, box), mb, "moments"), _check_stats(fin, x, box, mean_zero, mb, _ids(case)))
    print(f"RATIO mc_raw_movie_stats {_ids(case)}: {r:.3f}")
    worse(ratios, "mc_raw_movie_stats", r)


# ------------------------------------------------------------------ hot pixels: detection, list, moments, output


def _detect(calls, dev, rd, kind, gd, shape, box, thr, cap):
    check, ptr, stream_ptr = _api()
    t, h, w = shape
    stats = torch.full((t, 3), float("nan"), dtype=torch.float64, device=dev)
    hstats = torch.full((t, 3), float("nan"), dtype=torch.float64, device=dev)
    keys = torch.full((cap + 8,), -12345, dtype=torch.int64, device=dev)
    rv = torch.full((cap + 8, 2), float("nan"), dtype=torch.float32, device=dev)
    counter = torch.full((1,), -1, dtype=torch.int64, device=dev)
    counts = torch.full((t,), -1, dtype=torch.int32, device=dev)
    check(calls.mc_raw_hot_detect(ptr(rd), hr.KINDS[kind][0], ptr(gd), t, h, w, *box, thr, ptr(stats), ptr(hstats),
                                  ptr(keys), ptr(rv), cap, ptr(counter), ptr(counts), stream_ptr(dev)),
          "mc_raw_hot_detect")
    torch.cuda.synchronize()
    assert bool((keys[cap:] == -12345).all()) and bool(torch.isnan(rv[cap:]).all()), "wrote beyond the list's capacity"
    return stats, hstats, keys, rv, int(counter.item()), counts


@pytest.mark.parametrize("case", hr.HOT_CASES, ids=_ids)
def test_hot_detect_finalize_and_condition_hot_match_float64(calls, dev, ratios, case):
    check, ptr, stream_ptr = _api()
    kind, shape, thr = case
    t, h, w = shape
    N = h * w
    raw, gain, _ = hr.hot_movie(kind, shape)
    x = hr.product64(raw, gain)
    box = hr.central_box(h, w)
    rd, gd = _dev_view(raw, dev), _dev_view(gain, dev)
    stats, hstats, keys, rv, counter, counts = _detect(calls, dev, rd, kind, gd, shape, box, thr, 4096)
    hs = hstats.cpu().numpy()
    n = counter
    assert 0 < n <= 4096
    r_list, ref = hr.check_list(keys[:n].cpu().numpy(), rv[:n].cpu().numpy(), counts.cpu().numpy(), counter, raw, gain,
                                thr, hs[:, 0] / N, _ids(case))
    # before mc_raw_hot_finalize: the moments of the unreplaced frames, and the detection sums
    mb0 = hr.moment_bounds(x, box, True, 3, 8)
    r_mom = hr.assert_within(stats.cpu().numpy(), hr.moments64(x, box), mb0, "moments before finalize")
    hb = np.stack([mb0[:, 0], (6 * U + N * 2.0 ** -53) * (x * x).sum(axis=(1, 2))], axis=1)
    r_mom = max(r_mom, hr.assert_within(hs[:, :2], np.stack([x.sum(axis=(1, 2)), (x * x).sum(axis=(1, 2))], axis=1), hb,
                                        "detection sums"))
    sk, order = torch.sort(keys[:n], stable=True)
    srv = rv[:n][order].contiguous()
    assert np.array_equal(sk.cpu().numpy(), ref.keys)
    e_r = hr.replacement_error64(ref, x, thr)
    mb = hr.moment_bounds(x, box, True, 3, 8, ref, e_r)
    r_fin = 0.0
    for mean_zero in (1, 0):
        st = stats.clone()
        mu, sub, mean_rstd = torch.empty(t, device=dev), torch.empty(t, device=dev), torch.empty(2, device=dev)
        check(calls.mc_raw_hot_finalize(ptr(sk), ptr(srv), n, t, h, w, *box, mean_zero, ptr(hstats), ptr(st), ptr(mu),
                                        ptr(sub), ptr(mean_rstd), stream_ptr(dev)), "mc_raw_hot_finalize")
        torch.cuda.synchronize()
        assert np.array_equal(hstats.cpu().numpy(), hs), "mc_raw_hot_finalize changed hstats"
        r_fin = max(r_fin, hr.assert_within(st.cpu().numpy(), hr.moments64(ref.replaced, box), mb, "moments after finalize"))
        fin = dict(mu=mu.cpu().numpy(), sub=sub.cpu().numpy(), mean=float(mean_rstd[0]), rstd=float(mean_rstd[1]))
        r_fin = max(r_fin, _check_stats(fin, ref.replaced, box, mean_zero, mb, f"{_ids(case)} mean_zero={mean_zero}"))
    # mc_condition_movie_hot on the same movie, every pixel
    r_out = 0.0
    for mean_zero in (1, 0):
        cst = torch.empty(3 * t, dtype=torch.float64, device=dev)
        cnt = torch.full((t,), -1, dtype=torch.int32, device=dev)
        out = torch.full((t, h, w), float("nan"), dtype=torch.float32, device=dev)
        check(calls.mc_condition_movie_hot(ptr(rd), hr.KINDS[kind][0], ptr(gd), t, h, w, mean_zero, thr, ptr(cst), ptr(cnt),
                                           ptr(out), stream_ptr(dev)), "mc_condition_movie_hot")
        torch.cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy(), ref.counts)
        r_out = max(r_out, hr.check_condition_hot(out.cpu().numpy(), raw, gain, bool(mean_zero), thr,
                                                  f"mc_condition_movie_hot {_ids(case)} mean_zero={mean_zero}"))
    calls.ran("mc_raw_hot_detect", "mc_raw_hot_finalize", "mc_condition_movie_hot")
    print(f"RATIO hot {_ids(case)}: list {r_list:.3f} moments {r_mom:.3f} finalize {r_fin:.3f} output {r_out:.3f}")
    worse(ratios, "hot list r", r_list)
    worse(ratios, "hot moments", max(r_mom, r_fin))
    worse(ratios, "hot conditioned output", r_out)


def test_hot_route_through_the_engine_gives_the_same_list(calls, dev):
    """engine.RawMovie (mc_raw_hot_detect, the sort, mc_raw_hot_finalize) and engine.condition_movie on one case."""
    from torch_motion_correction_amd import engine

    kind, shape, thr = hr.HOT_CASES[0]
    t, h, w = shape
    raw, gain, _ = hr.hot_movie(kind, shape)
    x = hr.product64(raw, gain)
    rd, gd = torch.from_numpy(raw).to(dev), torch.from_numpy(gain).to(dev)
    for mean_zero in (True, False):
        rm = engine.RawMovie(rd, gd, mean_zero=mean_zero, hot_pixel_threshold=thr)
        torch.cuda.synchronize()
        ref = hr.hot64(x, thr)
        assert rm.n_hot == len(ref.keys) and np.array_equal(rm.hot_keys.cpu().numpy(), ref.keys)
        assert np.array_equal(rm.hot_counts.cpu().numpy(), ref.counts)
        box = hr.central_box(h, w)
        mb = hr.moment_bounds(x, box, True, 3, 8, ref, hr.replacement_error64(ref, x, thr))
        fin = dict(mu=rm.mu.cpu().numpy(), sub=rm.sub.cpu().numpy(), mean=float(rm.mean_rstd[0]), rstd=float(rm.mean_rstd[1]))
        _check_stats(fin, ref.replaced, box, int(mean_zero), mb, f"RawMovie mean_zero={mean_zero}")
        out, cnt = engine.condition_movie(rd, gd, mean_zero, hot_pixel_threshold=thr, return_hot_counts=True)
        torch.cuda.synchronize()
        hr.check_condition_hot(out.cpu().numpy(), raw, gain, mean_zero, thr, "condition_movie")
        assert np.array_equal(cnt.cpu().numpy(), ref.counts)
    calls.ran("mc_raw_hot_detect", "mc_raw_hot_finalize", "mc_condition_movie_hot", absent=("mc_raw_movie_stats",))


def test_hot_list_overflow_keeps_counting(calls, dev):
    kind, shape, thr = hr.HOT_CASES[0]
    t, h, w = shape
    raw, gain, _ = hr.hot_movie(kind, shape)
    cap = 16
    _, hstats, keys, rv, counter, counts = _detect(calls, dev, _dev_view(raw, dev), kind, _dev_view(gain, dev), shape,
                                                   hr.central_box(h, w), thr, cap)
    assert counter > cap
    hr.check_list(keys[:cap].cpu().numpy(), rv[:cap].cpu().numpy(), counts.cpu().numpy(), counter, raw, gain, thr,
                  hstats.cpu().numpy()[:, 0] / (h * w), "overflow", capacity=cap)
    calls.ran("mc_raw_hot_detect")


# ------------------------------------------------------------------ row corrections on hand-built lists


def _rows_case(h, w, full, variant):
    if full:
        nkx, y0, ny, g = w // 2 + 1, 0, h, None
    else:
        g = hr.rows_geometry(h, w)
        nkx, y0, ny = g.nkx, g.y0, g.ny
    keys, rv, (ym, xz, xf) = hr.rows_list(h, w, y0, ny, 13, single=variant == "single",
                                          skipped_first=variant != "first-in-window")
    mask = hr.rows_mask(h, w, ym, xz, xf) if (variant != "nomask" and not full) else None
    return keys, rv, mask, nkx, y0, ny, g


@pytest.mark.parametrize("variant", ["all", "nomask", "single", "first-in-window"])
@pytest.mark.parametrize("shape", hr.ROWS_SHAPES, ids=_ids)
def test_xc_rows_hot_correct_matches_float64(calls, dev, ratios, shape, variant):
    check, ptr, stream_ptr = _api()
    h, w = shape
    keys, rv, mask, nkx, y0, ny, g = _rows_case(h, w, False, variant)
    frame0, njobs, rstd = 1, 2, F32(0.21)
    T1 = hr._rng(5, h, w).normal(0, 3, (njobs, nkx, ny, 2)).astype(F32)
    guard = torch.full((T1.size + 64,), float("nan"), dtype=torch.float32, device=dev)
    Td = guard[32:32 + T1.size].view(T1.shape)
    Td.copy_(torch.from_numpy(T1))
    md = None if mask is None else torch.from_numpy(mask).to(dev)
    mean_rstd = torch.tensor([0.3, float(rstd)], dtype=torch.float32, device=dev)
    kd, rvd = torch.from_numpy(keys).to(dev), torch.from_numpy(rv).to(dev)  # named: they must outlive the launch
    check(calls.mc_xc_rows_hot_correct(ptr(kd), ptr(rvd), len(keys), frame0, njobs, h, w, ptr(md), ptr(mean_rstd), ptr(Td), g,
                                       stream_ptr(dev)), "mc_xc_rows_hot_correct")
    torch.cuda.synchronize()
    calls.ran("mc_xc_rows_hot_correct")
    gcpu = guard.cpu().numpy()
    assert np.isnan(gcpu[:32]).all() and np.isnan(gcpu[32 + T1.size:]).all(), "wrote outside T1"
    r = hr.check_rows(T1, Td.cpu().numpy(), keys, rv, mask, float(rstd), h, w, nkx, y0, ny, frame0, njobs,
                      f"mc_xc_rows_hot_correct {shape} {variant}")
    print(f"RATIO mc_xc_rows_hot_correct {shape} {variant}: {r:.3f}")
    worse(ratios, "mc_xc_rows_hot_correct", r)


@pytest.mark.parametrize("variant", ["all", "single", "first-in-window"])
@pytest.mark.parametrize("shape", hr.FULL_SHAPES, ids=_ids)
def test_full_rows_hot_correct_matches_float64(calls, dev, ratios, shape, variant):
    check, ptr, stream_ptr = _api()
    h, w = shape
    keys, rv, _, nkx, y0, ny, _ = _rows_case(h, w, True, variant)
    frame0, njobs = 1, 2
    pitch = calls.mc_full_spectrum_pitch(w)
    assert pitch > nkx  # elements beyond kx = w / 2 exist and must stay as they are
    S = hr._rng(6, h, w).normal(0, 3, (njobs, h, pitch, 2)).astype(F32)
    guard = torch.full((S.size + 64,), float("nan"), dtype=torch.float32, device=dev)
    Sd = guard[32:32 + S.size].view(S.shape)
    Sd.copy_(torch.from_numpy(S))
    kd, rvd = torch.from_numpy(keys).to(dev), torch.from_numpy(rv).to(dev)  # named: they must outlive the launch
    check(calls.mc_full_rows_hot_correct(ptr(kd), ptr(rvd), len(keys), frame0, njobs, h, w, ptr(Sd), pitch, stream_ptr(dev)),
          "mc_full_rows_hot_correct")
    torch.cuda.synchronize()
    calls.ran("mc_full_rows_hot_correct")
    gcpu = guard.cpu().numpy()
    assert np.isnan(gcpu[:32]).all() and np.isnan(gcpu[32 + S.size:]).all(), "wrote outside S"
    got = Sd.cpu().numpy()
    assert np.array_equal(got[:, :, nkx:], S[:, :, nkx:]), "the pitch's padding changed"
    # (njobs, h, kx, 2) -> the (njobs, kx, row, 2) layout of check_rows
    r = hr.check_rows(S[:, :, :nkx].transpose(0, 2, 1, 3), got[:, :, :nkx].transpose(0, 2, 1, 3), keys, rv, None, 1.0, h, w,
                      nkx, 0, h, frame0, njobs, f"mc_full_rows_hot_correct {shape} {variant}")
    print(f"RATIO mc_full_rows_hot_correct {shape} {variant}: {r:.3f}")
    worse(ratios, "mc_full_rows_hot_correct", r)


# ------------------------------------------------------------------ warp corrections


@pytest.mark.parametrize("case", hr.WARP_CASES, ids=_ids)
def test_warp_hot_corrections_match_float64(calls, dev, ratios, case):
    from torch_motion_correction_amd import engine

    check, ptr, stream_ptr = _api()
    kind, shape, thr = case
    t, h, w = shape
    raw, gain, _ = hr.hot_movie(kind, shape)
    x = hr.product64(raw, gain)
    ref = hr.hot64(x, thr)
    rm = engine.RawMovie(torch.from_numpy(raw).to(dev), torch.from_numpy(gain).to(dev), True, thr)
    assert np.array_equal(rm.hot_keys.cpu().numpy(), ref.keys)
    nbytes = C.c_int64(0)
    check(calls.mc_warp_rigid_scratch_bytes(t, h, w, C.byref(nbytes)), "mc_warp_rigid_scratch_bytes")
    scratch = torch.zeros((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)
    sd = torch.from_numpy(hr.WARP_SHIFTS).to(dev)
    st = stream_ptr(dev)
    check(calls.mc_warp_rigid_raw(ptr(rm.raw), rm.kind, ptr(rm.gain), ptr(rm.mu), t, h, w, ptr(sd), ptr(scratch), None, None,
                                  1, st), "mc_warp_rigid_raw tables")
    frames, total = engine.warp_rigid_raw(rm, None, 1.0, want_frames=True, want_sum=True, tables=(sd, scratch))
    torch.cuda.synchronize()
    calls.ran("mc_raw_hot_detect", "mc_raw_hot_finalize", "mc_warp_rigid_raw", "mc_warp_rigid_hot_taps", "mc_hot_scatter_add")
    assert calls.count("mc_hot_scatter_add") == 2  # frames and sum
    sc = scratch.cpu()
    Wy = sc[:t * h * 5].view(t, h, 5).numpy()
    Wx = sc[t * h * 5:t * 5 * (h + w)].view(t, 5, w).numpy()
    S = sc[t * 5 * (h + w):t * 5 * (h + w) + 2 * t].view(torch.int32).view(t, 2).numpy()
    # the records, from the kernel itself
    n = rm.n_hot
    rec_key = torch.full((49 * n,), -5, dtype=torch.int64, device=dev)
    rec_val = torch.full((49 * n,), float("nan"), dtype=torch.float32, device=dev)
    check(calls.mc_warp_rigid_hot_taps(ptr(rm.hot_keys), ptr(rm.hot_rv), n, t, h, w, ptr(scratch), ptr(rec_key),
                                       ptr(rec_val), st), "mc_warp_rigid_hot_taps")
    torch.cuda.synchronize()
    rv = rm.hot_rv.cpu().numpy()
    r_rec = hr.check_records(rec_key.cpu().numpy(), rec_val.cpu().numpy(), ref.keys, rv, Wy, Wx, S, h, w,
                             f"mc_warp_rigid_hot_taps {_ids(case)}")
    # frames and sum against the float64 rigid resample of the REPLACED movie
    mu = rm.mu.cpu().numpy()
    rep32 = hr.product64(raw, gain)
    rep32.reshape(-1)[ref.keys] = rv[:, 0].astype(np.float64)  # the kernel's own replacements: their accuracy is check_list's
    want, _ = rigid_resample_gather_stack(lambda f: rep32[f] - float(mu[f]), hr.WARP_SHIFTS)
    ref_un, mag, err, wterm = rigid_resample_gather_stack(
        lambda f: condition_float64(raw[f], gain, mu[f]), hr.WARP_SHIFTS,
        extra=lambda f: conditioning_error(raw[f], gain, mu[f]), weight_error=True)
    _, rec_bound = hr.warp_correction64(ref.keys, rv, Wy, Wx, S, h, w)
    base = 32 * U * mag + wterm + err            # test_rigid_kernels_float64's bound of the kernel's own resampling
    # mc_hot_scatter_add: a run of cnt records (verified above) within cnt u sum|val|, and the addition onto the output
    rk, rval = rec_key.cpu().numpy(), rec_val.cpu().numpy().astype(np.float64)
    cnt, absval = np.zeros(t * h * w), np.zeros(t * h * w)
    np.add.at(cnt, rk[rk != hr.HOT_NONE], 1)
    np.add.at(absval, rk[rk != hr.HOT_NONE], np.abs(rval[rk != hr.HOT_NONE]))
    cnt, absval = cnt.reshape(t, h, w), absval.reshape(t, h, w)
    bound = base + rec_bound + cnt * U * absval + U * (cnt > 0) * (np.abs(ref_un) + base + absval)
    assert (want != 0).any() and cnt.max() >= 2
    r_frames = assert_frames(frames, want, bound, f"frames {_ids(case)}")
    cs, as_ = cnt.sum(0), absval.sum(0)
    sum_bound = ((base + rec_bound).sum(0) + t * U * np.abs(ref_un).sum(0)   # the rigid tests' sum bound
                 + cs * U * as_ + U * (cs > 0) * (np.abs(ref_un).sum(0) + base.sum(0) + as_))
    r_sum = hr.assert_within(total.cpu().numpy(), want.sum(0), sum_bound, f"sum {_ids(case)}")
    print(f"RATIO warp hot {_ids(case)}: records {r_rec:.3f} frames {r_frames:.3f} sum {r_sum:.3f}")
    worse(ratios, "warp records", r_rec)
    worse(ratios, "warp frames", r_frames)
    worse(ratios, "warp sum", r_sum)


def test_hot_scatter_add_on_hand_built_runs(calls, dev, ratios):
    check, ptr, stream_ptr = _api()
    lists, limit, out = hr.scatter_case()
    for keys, vals in lists:
        guard = torch.full((limit + 64,), float("nan"), dtype=torch.float32, device=dev)
        od = guard[32:32 + limit]
        od.copy_(torch.from_numpy(out))
        kd, vd = torch.from_numpy(keys).to(dev), torch.from_numpy(vals).to(dev)  # named: they must outlive the launch
        check(calls.mc_hot_scatter_add(ptr(kd), ptr(vd), len(keys), limit, ptr(od), stream_ptr(dev)), "mc_hot_scatter_add")
        torch.cuda.synchronize()
        g = guard.cpu().numpy()
        assert np.isnan(g[:32]).all() and np.isnan(g[32 + limit:]).all(), "wrote outside out"
        r = hr.check_scatter(out, od.cpu().numpy(), keys, vals, limit, "mc_hot_scatter_add")
        print(f"RATIO mc_hot_scatter_add m={len(keys)}: {r:.3f}")
        worse(ratios, "mc_hot_scatter_add", r)
    calls.ran("mc_hot_scatter_add")
