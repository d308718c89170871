"""Host checks of tests/xc_reference.py -- the float64 definitions of the cross-correlation estimate's stages, the
derived bounds and the case tables of tests/test_xc_kernels_float64.py -- without a GPU: the reference against
tests/global_refine_reference.py where the two overlap and against planted drifts, the fp32 CPU oracle INSIDE every
bound on every table case (a bound the oracle broke would be a wrong bound), the conditions that keep the arg-max
criterion sharp (a unique float64 maximum by more than 2E on the planted cases; no gap and 2 .. MAX_TIES admissible
positions on the constructed near-tie cases; at most MAX_TIES on pure noise), and deliberately wrong stand-ins that every comparison helper must reject.
The raw patch row pass (mc_xc_rows_forward_dual_raw) has its own section: an fp32 restatement on the input the GPU
test uses (xc_reference.raw_patch_input) inside the same bounds, the faults its RAW branch could make -- a gain
column, the gain offset without the modulo, the other frame's subtrahend, a sample to the left, an unsigned i16
half, the exponents exchanged -- each outside them, and the clamped loads shown to be an addressing matter only.

The oracle's worst ratio per family is printed as `RATIO ...` (run with -s); those figures are the last column of
the table in tests/test_xc_kernels_float64.py."""

import math

import numpy as np
import pytest
import torch

import xc_reference as xr
from conftest import drift_stack
from global_refine_reference import filtered_spectra
from oracle import motion as om

U = xr.U


def _oracle_spectra(x, pa, jobs=None, expo=None):
    """The oracle's own fp32 op sequence (oracle.motion.estimate_global_motion / the patch loop) for the filtered
    spectra of whole frames or of windows with a mask exponent, pruned to the kept bins -> (njobs, nkx, nky)."""
    h, w, ps, b, band = pa
    xn = om.normalize_image(x.float())
    mask, benv, bandf = om._filters((h, w), ps, b, band)
    g = xr.geometry(pa)
    rows = torch.from_numpy(xr.kept_rows(g))
    if jobs is None:
        jobs, expo = [(f, 0, 0) for f in range(x.shape[0])], [1] * x.shape[0]
    out = []
    for (f, y0, x0), e in zip(jobs, expo):
        win = xn[f, y0:y0 + h, x0:x0 + w].clone()
        for _ in range(e):
            win *= mask  # in place, as the patch loop's repeated `cur *= mask` on the memo entry
        spec = torch.fft.rfftn(win, dim=(-2, -1)) * bandf * benv
        out.append(spec[rows][:, :g.nkx].T)
    return torch.stack(out)


# ------------------------------------------------------------------ the reference itself


@pytest.mark.parametrize("case", [(3, 64, 64, 1.0), (2, 100, 120, 0.83), (2, 121, 135, 2.5)])
def test_spectra_and_map_agree_with_the_refinement_reference(case):
    t, h, w, ps = case
    pa = xr.args(h, w, ps)
    x = xr.noise(t, h, w, mean=5.0, std=2.0)
    S = xr.spectra64(x, pa)
    full = filtered_spectra(x, ps)
    g = xr.geometry(pa)
    assert np.abs(S - np.transpose(full[:, xr.kept_rows(g)][:, :, :g.nkx], (0, 2, 1))).max() <= 1e-9 * np.abs(full).max()
    for f in range(t):
        assert np.abs(xr.full_spectrum(S[f], pa) - full[f]).max() <= 1e-9 * np.abs(full).max()  # nothing kept is pruned
    cc = xr.correlation64(S[1], S[0], pa)
    want = np.fft.irfft2(np.conj(full[0]) * full[1], s=(h, w))
    assert np.abs(cc - want).max() <= 1e-12 * np.abs(want).max()


def test_integer_peaks_are_the_planted_drifts():
    x, dy, dx = drift_stack(8, 256, 256)
    pa = xr.args(256, 256)
    S = xr.spectra64(x, pa)
    for f in range(8):
        cc = xr.correlation64(S[f], S[4], pa)
        assert xr.shifts64(np.argmax(cc), (256, 256)) == (int(dy[f] - dy[4]), int(dx[f] - dx[4]))
    x = xr.planted(3, 128, 160, [(5, -7), (0, 0), (-12, 14)])
    S = xr.spectra64(x, xr.args(128, 160))
    assert xr.shifts64(np.argmax(xr.correlation64(S[0], S[1], xr.args(128, 160))), (128, 160)) == (5, -7)
    assert xr.shifts64(np.argmax(xr.correlation64(S[2], S[1], xr.args(128, 160))), (128, 160)) == (-12, 14)


def test_neighbourhood_is_not_circular_and_offsets_follow_the_guards():
    cc = np.arange(20.0).reshape(4, 5)
    nb = xr.neighbourhood64(cc, 0)
    assert np.isnan(nb[0]).all() and np.isnan(nb[:, 0]).all() and nb[1, 1] == 0 and nb[2, 2] == 6
    nb = xr.neighbourhood64(cc, 19)
    assert np.isnan(nb[2]).all() and np.isnan(nb[:, 2]).all() and nb[0, 0] == 13
    assert xr.offsets64(nb) == (0.0, 0.0)
    q = np.array([[0, 1.0, 0], [2.0, 5.0, 2.0], [0, 3.0, 0]])
    oy, ox = xr.offsets64(q)
    assert ox == 0.0 and oy == pytest.approx(0.5 * (1 - 3) / (1 - 10 + 3))


def test_accumulate64_is_the_oracles_sub_pixel_and_rejection():
    """accumulate64 against the oracle's _sub_pixel + wrap + _reject_outliers on random neighbourhoods."""
    rng = np.random.default_rng(3)
    P, npatch, t = 48, 12, 4
    peaks = rng.integers(0, P * P, size=2 * npatch)
    peaks[:6] = [0, P - 1, 5 * P, 5 * P + P - 1, (P - 1) * P + 7, 24 * P + 25]
    peaks[8] = 40 * P + 3  # an outlier among small shifts
    peaks[6:8] = [2 * P + 3, 3 * P + 2]
    peaks[9:12] = [1 * P + 1, 2 * P + 2, 3 * P + 1]
    cc3 = rng.standard_normal((2 * npatch, P, P)).astype(np.float32)
    for p in range(2 * npatch):
        cc3[p].reshape(-1)[peaks[p]] = 9.0
    nb = np.stack([xr.neighbourhood64(cc3[p], peaks[p]) for p in range(2 * npatch)])
    field, _ = xr.accumulate64(peaks, nb, [3, 1], npatch, P, t, 1.3, 2.0, 3)
    for fi, frame in enumerate((3, 1)):
        sl = slice(fi * npatch, (fi + 1) * npatch)
        py, px = om._sub_pixel(torch.from_numpy(cc3[sl]), torch.from_numpy(peaks[sl]), P, P)
        sy = torch.where(py <= P // 2, py, py - P)
        sx = torch.where(px <= P // 2, px, px - P)
        sy, sx = om._reject_outliers(sy, sx, 2.0)
        assert np.abs(field[0, frame] - (sy * 1.3).numpy()).max() <= 1e-5
        assert np.abs(field[1, frame] - (sx * 1.3).numpy()).max() <= 1e-5
    assert not field[:, [0, 2]].any()


# ------------------------------------------------------------------ the fp32 oracle inside every bound


SPECTRA_CASES = xr.SPECTRA_SMALL + xr.SPECTRA_WIDE + xr.SPECTRA_LINES + [xr.WIDE_BAND, xr.BENCH]


@pytest.mark.parametrize("case", SPECTRA_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-{c[3]}-{c[4][1]:g}")
def test_oracle_spectra_stay_inside_the_bound(case):
    t, h, w, ps, band = case
    pa = xr.args(h, w, ps, band)
    x = xr.noise(t, h, w, mean=5.0, std=2.0)
    parts = xr.spectra_parts(x, pa)
    b = xr.spectra_bounds(pa, parts["mean"], parts["std"])
    r = xr.check_spectra(_oracle_spectra(x, pa), parts, b, f"oracle {case[:3]}")
    print(f"RATIO oracle spectra {case[:3]} ps {ps} band {band} ({b['kinds']}): L2 {r[0]:.3f} bin {r[1]:.3f}")


@pytest.mark.parametrize("mean,std", xr.STAT_INPUTS)
def test_oracle_spectra_with_an_offset_stay_inside_the_bound(mean, std):
    pa = xr.args(256, 256)
    x = xr.noise(2, 256, 256, mean=mean, std=std)
    parts = xr.spectra_parts(x, pa)
    b = xr.spectra_bounds(pa, parts["mean"], parts["std"])
    r = xr.check_spectra(_oracle_spectra(x, pa), parts, b, f"oracle N({mean}, {std}^2)")
    print(f"RATIO oracle spectra N({mean:g}, {std:g}^2): L2 {r[0]:.3f} bin {r[1]:.3f}")


@pytest.mark.parametrize("p", [48, 63, 80, 1024])
def test_oracle_patch_spectra_stay_inside_the_bound(p):
    """Windows at origins that are no multiple of 4 samples, mask exponents 1, 2 and 3."""
    H, W = (p + 9, p + 14)
    x = xr.noise(2, H, W, mean=5.0, std=2.0)
    jobs, expo = [(0, 1, 3), (1, 7, 13), (0, 9, 6), (1, 0, 1)], [1, 2, 3, 1]
    pa = xr.args(p, p)
    parts = xr.spectra_parts(x, pa, jobs, expo)
    bs = [xr.spectra_bounds(pa, parts["mean"], parts["std"], expo=e) for e in expo]
    r = xr.check_spectra(_oracle_spectra(x, pa, jobs, expo), parts, bs, f"oracle patches {p}")
    print(f"RATIO oracle patch spectra {p}: L2 {r[0]:.3f} bin {r[1]:.3f}")


# ------------------------------------------------------------------ raw patch jobs: the fp32 restatement and planted faults


def _raw_patch_fp32(kind, h, sub, rstd, ex, fault=None, clamp=None, chords=True):
    """The raw patch row pass + column pass (mc_xc_rows_forward_dual_raw, mc_xc_cols_forward) restated in fp32 torch on
    the CPU for xr.RAW_PATCH_JOBS of xr.raw_patch_input(kind, h): per job the window of raw counts and of the gain
    at the job's offset within its frame, (float32(raw) * gain - sub[frame]) * rstd with one rounding per operation
    (no fma), times mask^e as a product of e factors, fp32 rfft2, the kept bins, the fp32 filter -> (njobs, nkx, nky).

    `fault`: one deliberate error of the classes the kernel's RAW branch could make (the test below names them).
    `clamp`: the kernel's addressing instead of the plain window -- a pair of samples at the even window column p is
    read at min(max(p, xlo), xhi), xlo / xhi the row's chord (`chords`) or the mask's bounding columns, and rows
    outside the mask's rows are not read at all; 'both' as the kernel, 'left' with the clamp on the right omitted."""
    from torch_motion_correction_amd import plan

    raw, gain = xr.raw_patch_input(kind, h)
    _, H, W = raw.shape
    pa = xr.args(h, 1024)
    mask, benv, bandf = om._filters((h, 1024), pa[2], pa[3], pa[4])
    g = xr.geometry(pa)
    rows = torch.from_numpy(xr.kept_rows(g))
    area = H * W
    rflat = raw.reshape(-1)
    gflat = gain.reshape(-1)
    if fault == "gain without the modulo":  # what lies past the gain's end: modelled as the gain one row further down
        gflat = torch.cat([gflat, gflat.roll(-W)])
    sub = torch.from_numpy(np.asarray(sub, dtype=np.float32))
    rstd = torch.tensor(float(rstd), dtype=torch.float32)
    if clamp:
        p = torch.arange(1024) & ~1
        if chords:
            ch = plan.row_chords(mask).long()
            xlo, xhi = ch[:, 0:1], ch[:, 1:2] + 2
        else:
            xlo, xhi = torch.full((h, 1), g.x0), torch.full((h, 1), g.x1 - 2)
        lo = torch.minimum(torch.maximum(p[None, :], xlo), xhi)
        src = (lo if clamp == "both" else torch.maximum(p[None, :], xlo)) + (torch.arange(1024) & 1)[None, :]
        live = torch.zeros(h, 1, dtype=torch.bool)
        live[g.y0:g.y0 + g.ny] = True
        assert not bool(mask[src != torch.arange(1024)[None, :]].any()) and not bool(mask[~live[:, 0]].any())
    out = []
    for (f, y0, x0), e in zip(xr.RAW_PATCH_JOBS, ex):
        off = f * area + y0 * W + x0
        goff = off if fault == "gain without the modulo" else off % area
        if fault == "gain one column to the right":
            goff += 1
        if fault == "raw window one sample to the left":
            off -= 1
        win = torch.as_strided(rflat, (h, 1024), (W, 1), off)
        gwin = torch.as_strided(gflat, (h, 1024), (W, 1), goff)
        if clamp:
            win, gwin = torch.gather(win, 1, src), torch.gather(gwin, 1, src)
        x = win.float()
        if fault == "i16 high half widened unsigned":
            x[:, 1::2] = (win[:, 1::2].int() & 0xffff).float()
        s = sub[1 - f] if fault == "sub of the other frame" else sub[f]
        c = (x * gwin - s) * rstd
        pw = mask.clone()
        for _ in range(e - 1):
            pw = pw * mask
        c = c * pw
        if clamp:
            c = torch.where(live, c, torch.zeros(()))
        spec = torch.fft.rfftn(c, dim=(-2, -1)) * bandf * benv
        out.append(spec[rows][:, :g.nkx].T)
    return torch.stack(out)


def _raw_patch_case(kind, h):
    """-> (sub, rstd, pa, [(exponents, parts, bounds) of the dual form's two spectra])."""
    raw, gain = xr.raw_patch_input(kind, h)
    sub, rstd = xr.raw_stats64(raw, gain)
    pa = xr.args(h, 1024)
    return sub, rstd, pa, [(ex,) + xr.raw_patch_reference(kind, pa, sub, rstd, ex) for ex in xr.RAW_PATCH_EXPO]


@pytest.mark.parametrize("h", xr.RAW_PATCH_HEIGHTS)
@pytest.mark.parametrize("kind", ["u8", "i16"])
def test_raw_patch_restatement_stays_inside_the_bound(kind, h):
    """The conditions of the raw patch test -- a gain of dynamic range 16, a second frame brighter by more than a
    quarter of the mean, i16 counts negative in both halves of a pair, odd origins on an odd frame width -- are
    satisfiable: a correct fp32 computation of the same jobs stays inside the bounds the kernel is held to, on the
    1024 x 1024 window (ny = 800) and on the 16 x 1024 one (ny = 16: the plan whose ny % 32 != 0)."""
    xr.check_raw_patch_jobs(h)
    sub, rstd, pa, refs = _raw_patch_case(kind, h)
    g = xr.geometry(pa)
    assert (g.ny % 32 == 0) == (h == 1024) and g.ny % 8 == 0 and g.nkx <= 128 and g.W == 1024
    assert float(sub[1] - sub[0]) * float(rstd) >= 0.25  # the other frame's subtrahend: a quarter of a std, >> any bound
    for tag, (ex, parts, bounds) in zip("ab", refs):
        assert float(sub[1] - sub[0]) * float(rstd) >= 1e4 * max(b["rel"] for b in bounds)
        r = xr.check_spectra(_raw_patch_fp32(kind, h, sub, rstd, ex), parts, bounds, f"raw patch restatement {kind} {h} {tag}")
        print(f"RATIO oracle raw patch jobs {h} {kind} {tag} (ny {g.ny}; conditioning {bounds[0]['conditioning'] / U:.1f} u of "
              f"{bounds[0]['rel'] / U:.0f} u): L2 {r[0]:.3f} bin {r[1]:.3f}")


RAW_FAULTS = ["gain one column to the right", "gain without the modulo", "sub of the other frame",
              "raw window one sample to the left", "i16 high half widened unsigned", "ea and eb exchanged"]


@pytest.mark.parametrize("kind,fault", [(k, f) for k in ("u8", "i16") for f in RAW_FAULTS if k == "i16" or not f.startswith("i16")])
def test_raw_patch_planted_faults_are_caught(kind, fault):
    """Each error the RAW branch could make, planted into the restatement, leaves the bound -- on the spectrum of
    mask^ea and on that of mask^eb.  (Unsigned widening of the high half is an i16 matter; u8 has no such half.)"""
    sub, rstd, pa, refs = _raw_patch_case(kind, 1024)
    for i, (ex, parts, bounds) in enumerate(refs):
        wrong_ex = xr.RAW_PATCH_EXPO[1 - i] if fault == "ea and eb exchanged" else ex
        S = _raw_patch_fp32(kind, 1024, sub, rstd, wrong_ex, fault=fault)
        with pytest.raises(AssertionError, match="job"):
            xr.check_spectra(S, parts, bounds, f"{fault} {kind} {'ab'[i]}")


@pytest.mark.parametrize("chords", [True, False])
def test_raw_patch_clamp_is_only_an_addressing_matter(chords):
    """The kernel reads a pair outside its row's chord (or the mask's bounding columns) at the clamped address; the
    mask is exactly 0 there, so which sample it reads cannot matter.  Stated as a test: the restatement with the
    kernel's clamped reads, with the clamp on the right omitted (the unclamped sample where the mask is 0) and with
    plain window reads give the same spectra, all inside the bound -- this 'fault' must NOT be seen."""
    sub, rstd, pa, refs = _raw_patch_case("i16", 1024)
    ex, parts, bounds = refs[0]
    plain = _raw_patch_fp32("i16", 1024, sub, rstd, ex)
    for clamp in ("both", "left"):
        S = _raw_patch_fp32("i16", 1024, sub, rstd, ex, clamp=clamp, chords=chords)
        assert torch.equal(S, plain), clamp
    xr.check_spectra(plain, parts, bounds, f"clamp chords={chords}")


MAP_CASES = ([(c, k) for c in xr.MAP_SEPARATE + xr.MAP_FUSED for k in ("small", "large", "noise", "tie", "border")]
             + [(c, "near") for c in xr.MAP_FUSED])


def _near_rows(h, w):
    """Rows the near-window search stores per end of the map: host arithmetic of libmcorr (no device is touched)."""
    from torch_motion_correction_amd import _lib

    return int(_lib.load().mc_xc_near_rows(xr.geometry(xr.args(h, w))))


@pytest.mark.parametrize("case,kind", MAP_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_oracle_map_peak_neighbourhood_and_parabola_stay_inside_the_bounds(case, kind):
    """oracle.estimate_global_motion(return_cc=True): its fp32 map within E of cc64 and rel_C in L2, its arg-max
    admissible, its 3 x 3 values and parabola offsets inside their bounds; and the conditions on the inputs, per
    pair: a unique maximum by more than 2E on the planted cases; on the near-tie cases (xc_reference.tied) a gap
    top1 - top2 of at most 2E with 2 .. MAX_TIES admissible positions -- the tolerant branch of the criterion, on
    every path; on pure noise at most MAX_TIES admissible positions (white noise almost never ties within 2E: most
    of its pairs have a unique maximum, and nothing is claimed of their gap)."""
    t, h, w = case
    x, pa, _, pairs = xr.map_reference(t, h, w, kind, _near_rows(h, w) if kind == "near" else None)
    field, ccs = om.estimate_global_motion(x, 1.0, return_cc=True)
    worst = [0.0] * 4
    for f, cc64, rel_c, E in pairs:
        what = f"oracle {case} {kind} frame {f}"
        cc = ccs[f].numpy()
        m = xr.check_map(cc, cc64, rel_c, E, what)
        p = int(np.argmax(cc))
        a = xr.check_peak(p, (float(field[0, f, 0, 0]), float(field[1, f, 0, 0])), cc64, E, what)
        n = xr.check_neighbourhood(xr.neighbourhood64(cc, p), cc64, p, E, what)
        o = xr.check_offsets(xr.neighbourhood64(cc, p), cc64, p, E, what)
        worst = [max(u, v) for u, v in zip(worst, (m[0], m[1], n, o))]
        adm = xr.admissible(cc64, E)
        flat = np.sort(cc64.reshape(-1))
        if kind == "noise":
            assert 1 <= len(adm) <= xr.MAX_TIES, f"{what}: {len(adm)} positions within 2E of the maximum: another seed"
            print(f"  {what}: top1 - top2 = {flat[-1] - flat[-2]:.3e}, 2E = {2 * E:.3e}, admissible {len(adm)}")
        elif kind == "tie":  # the tolerant branch: no gap, and still only a few admissible positions
            assert flat[-1] - flat[-2] <= 2 * E, f"{what}: top1 - top2 = {flat[-1] - flat[-2]:.3e} > 2E = {2 * E:.3e}"
            assert 2 <= len(adm) <= xr.MAX_TIES, f"{what}: {len(adm)} positions within 2E of the maximum"
            assert p in adm
        else:
            assert len(adm) == 1 and adm[0] == p, f"{what}: the planted maximum is not unique by 2E ({len(adm)} admissible)"
    print(f"RATIO oracle map {case} {kind}: L2 {worst[0]:.3f} value {worst[1]:.3f} nb {worst[2]:.3f} parabola {worst[3]:.3f}")


# ------------------------------------------------------------------ the checks can fail


@pytest.fixture(scope="module")
def standin():
    t, h, w = 5, 256, 256
    x, pa, parts, pairs = xr.map_reference(t, h, w, "small")
    b = xr.spectra_bounds(pa, parts["mean"], parts["std"])
    return pa, parts, b, pairs


def test_the_exact_spectrum_and_map_pass(standin):
    pa, parts, b, pairs = standin
    assert xr.check_spectra(parts["S"], parts, b, "exact") == (0.0, 0.0)
    f, cc64, rel_c, E = pairs[0]
    p = int(np.argmax(cc64))
    xr.check_map(cc64, cc64, rel_c, E, "exact")
    xr.check_peak(p, xr.shifts64(p, cc64.shape), cc64, E, "exact")
    xr.check_neighbourhood(xr.neighbourhood64(cc64, p), cc64, p, E, "exact")


def test_rejects_one_kept_bin_scaled(standin):  # (a)
    pa, parts, b, _ = standin
    S = parts["S"].copy()
    k = np.argwhere(parts["filt"] != 0)[len(np.argwhere(parts["filt"] != 0)) // 2]
    S[0, k[0], k[1]] *= 1 + 1e-4
    with pytest.raises(AssertionError, match="bin"):
        xr.check_spectra(S, parts, b, "a")


def test_rejects_weak_bins_off_by_1e_3():  # (b)
    """The weakest 10 % of the kept bins -- by filter weight, under a B factor of 5000 A^2 that takes the envelope
    down to 4e-6 at the band edge -- off by 1e-3 relative: under the max-norm metric of the existing test
    (max |S - ref| / max |ref| <= 2e-6) this stand-in passes; weighed against each bin's own filter value it fails."""
    pa = (256, 256, 1.0, 5000.0, xr.DEFAULT_BAND)
    parts = xr.spectra_parts(xr.noise(1, 256, 256), pa)
    b = xr.spectra_bounds(pa, parts["mean"], parts["std"])
    S = parts["S"].copy()
    kept = np.argwhere(parts["filt"] != 0)
    weak = kept[np.argsort(parts["filt"][kept[:, 0], kept[:, 1]])[:len(kept) // 10]]
    S[0][weak[:, 0], weak[:, 1]] *= 1 + 1e-3
    assert np.abs(S[0] - parts["S"][0]).max() / np.abs(parts["S"][0]).max() <= 2e-6
    assert xr.check_spectra(parts["S"], parts, b, "b exact") == (0.0, 0.0)
    with pytest.raises(AssertionError, match="bin"):
        xr.check_spectra(S, parts, b, "b")


def test_rejects_a_non_zero_filtered_out_bin(standin):  # (f)
    pa, parts, b, _ = standin
    S = parts["S"].copy()
    k = np.argwhere(parts["filt"] == 0)[0]
    S[1, k[0], k[1]] = 1e-30
    with pytest.raises(AssertionError, match="not exactly zero"):
        xr.check_spectra(S, parts, b, "f")


def test_rejects_a_map_with_a_row_group_shifted(standin):  # (c)
    _, _, _, pairs = standin
    f, cc64, rel_c, E = pairs[0]
    cc = cc64.copy()
    cc[64:80] = cc64[65:81]
    with pytest.raises(AssertionError):
        xr.check_map(cc, cc64, rel_c, E, "c")


def test_rejects_a_peak_one_pixel_away(standin):  # (d)
    _, _, _, pairs = standin
    for f, cc64, _, E in pairs:
        p = int(np.argmax(cc64))
        for q in (p + 1, p - 1, p + cc64.shape[1], p - cc64.shape[1]):
            with pytest.raises(AssertionError):
                xr.check_peak(q % cc64.size, None, cc64, E, "d")
        with pytest.raises(AssertionError, match="shift"):
            xr.check_peak(p, (0.0, 1.0e9), cc64, E, "d")
        with pytest.raises(AssertionError, match="not an index"):
            xr.check_peak(cc64.size, None, cc64, E, "d")


def test_rejects_a_transposed_neighbourhood(standin):  # (e)
    _, _, _, pairs = standin
    f, cc64, _, E = pairs[0]
    p = int(np.argmax(cc64))
    nb = xr.neighbourhood64(cc64, p)
    with pytest.raises(AssertionError):
        xr.check_neighbourhood(nb.T.copy(), cc64, p, E, "e")
    with pytest.raises(AssertionError):
        xr.check_offsets(nb.T.copy(), cc64, p, E, "e")
    bad = nb.copy()
    bad[0, 0] = np.nan
    with pytest.raises(AssertionError, match="NaN pattern"):
        xr.check_neighbourhood(bad, cc64, p, E, "e")


def test_bounds_are_built_from_the_plans_line_kinds():
    """Each line's kind comes from the plan: native powers of two, direct 2880-point lines, chirp-z otherwise, and
    the bound grows with the transform (no constant fitted to anything)."""
    kinds = lambda h, w: xr.line_costs(xr.geometry(xr.args(h, w)))["kinds"]
    assert kinds(256, 256) == {"rows": "native", "cols": "native"}
    assert kinds(96, 5760)["rows"] == "direct" and kinds(2880, 128)["cols"] == "direct"
    assert "chirp-z" in kinds(100, 120)["rows"] and "chirp-z" in kinds(100, 120)["cols"]
    assert "M=10240" in kinds(4100, 128)["cols"] and "M=16384" in kinds(5200, 128)["cols"] and "M=5120" in kinds(96, 7000)["rows"]
    rel = lambda h, w, **k: xr.spectra_bounds(xr.args(h, w), 0.0, 1.0, **k)["rel"]
    assert rel(64, 64) < rel(256, 256) < rel(4096, 4096) < 250 * U
    assert rel(256, 256, expo=2) > rel(256, 256) and rel(256, 256, conditioning=1e-6) == pytest.approx(rel(256, 256) + 1e-6)
    mh = xr.mask_spectrum64(xr.args(256, 256))
    f0 = xr.spectra_bounds(xr.args(256, 256), 0.0, 1.0, fused=(0.0, mh))
    f33 = xr.spectra_bounds(xr.args(256, 256), 0.0, 1.0, fused=(33.0, mh))
    assert f0["rel"] == pytest.approx(rel(256, 256)) and f0["fix_l2"] == 0.0 and f33["rel"] > 20 * f0["fft"]
    assert math.isinf(xr.parabola_bound(1.0, 1.0, 1.0, 1e-3)) and xr.parabola_bound(0.0, 1.0, 0.0, 1e-3) == pytest.approx(1e-3 / (2 - 4e-3))
