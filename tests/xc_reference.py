"""Shared pieces of the cross-correlation estimate's tests (tests/test_xc_reference_host.py and
tests/test_xc_kernels_float64.py): every stage of the estimate in float64 by its definition -- filtered spectra on
the kept bins, correlation map, 3 x 3 neighbourhood, parabola, field accumulation -- and the error bound of each
stage, derived rounding by rounding from the unit roundoff of fp32 and the pass list of every line.

TEST INFRASTRUCTURE ONLY: numpy / torch on the CPU, fp32 (fp16, conditioned raw) inputs at their float64 value,
float64 arithmetic, numpy's FFT.  Nothing here calls into the HIP path; `plan` is used for the host-side geometry
(which bins are kept, which kind of line transforms an axis) only.  No constant is measured on a kernel.

Reused: global_refine_reference.filtered_spectra / wrap / parabola_offset (the mask and filter tables are the
oracle's, evaluated as the oracle evaluates them and widened), fourier_reference's U, ETA, C_MUL, GAMMA, CAP, measure
and its per-line cost functions, rigid_reference.condition_float64 / conditioning_error for raw input.

THE BOUNDS (u = 2^-24; all first order, the passes of a transform are unitary up to scale so their relative L2
errors add, Higham section 24.1):

  rel_S   relative L2 error of one job's filtered spectrum on the kept bins,
            rel_S = norm + mask + rows_fwd + cols_fwd + filter
          norm    x_n = (x - mean) rstd: the fp32 mean is off by u |mean| -- a constant offset, relative to the unit
                  variance of x_n: u |mean| / std; the subtraction rounds once (u), rstd is a rounded fp32 value whose
                  fp32 evaluation (root, reciprocal) rounds twice more (3u), the product rounds once (u):
                  (5 + |mean| / std) u.
          mask    the mask table is an fp32 raised cosine cos(pi/2 * d / s): the constant, the quotient and the product
                  round (3u of an angle <= pi / 2: 4.7u absolute), the cosine is good to an ulp (u absolute):
                  <= 6u absolute, and only on the soft ring 0 < mask < 1.  Against the unit-variance samples that is
                  6u sqrt(#ring / sum mask^2e) relative, e times for mask^e, plus the e products (e u).
          rows_fwd, cols_fwd   the pass list of that axis' line kind (line_costs): log2(n) eta for a power of two --
                  whatever radix the kernel nests them in -- + eta for the packed-real butterfly of an even width;
                  fourier_reference._line_cost for direct mixed-radix and chirp-z lines (with the output pruning
                  the forward row pass asks for).
          filter  the product with the filter rounds once (u); the filter table is exp(-B f^2 / (4 ps^2)) in fp32 on
                  either side: f from two products, a sum and a root (<= 3u relative), f / ps, its square, B times,
                  / 4 (exact): the exponent E carries (2 * 4 + 2) u = 10u relative, i.e. 10 |E| u of the value, and
                  expf an ulp (2u).  The reference table is the CPU's fp32 evaluation, the kernels' table another:
                  they are at most twice that apart: u + 2 (10 |E|max + 2) u.
          raw     u8 / i16 input adds rigid_reference.conditioning_error in L2, relative to the conditioned job.
          fp16    the exact up-cast: nothing.
          The fused-statistics route transforms (x - m0) mask and finishes by linearity, S = filt rstd (Y - (mean -
          m0) Mhat): the transform's error is relative to ||Y||, which is sqrt(1 + d^2) times the norm of the
          normalised job's spectrum, d = |mean - m0| / std; Mhat carries its own forward error (rows_fwd + cols_fwd)
          and the fix-up two more roundings (the product, the difference: 2u), all scaled by d: in L2
          d (rows_fwd + cols_fwd + 2u) ||filt Mhat||, per bin d (rows_fwd + cols_fwd + 2u) CAP filt[bin] |Mhat[bin]|.
          With m0 within a few std / sqrt(n) of the mean d is ~0.1 and both are small; with m0 = 0 on N(1000, 30^2)
          d = 33 and the route would lose five bits -- the claim the N(1000, 30^2) case tests.

          Statements: ||S - S64||_2 <= rel_S ||S64||_2 over the kept bins (+ the fix-up's L2 term); every bin with a
          non-zero filter value |S - S64| <= CAP rel_S filt[bin] rms(unfiltered spectrum of the job) (+ the fix-up's
          per-bin term); every bin the filter sets to zero is exactly 0.  The rms of the unfiltered spectrum is
          taken over ALL H x W bins, by Parseval ||x_n mask^e||_2: the rounding error of a transform lands on every
          bin alike, whether the bin is kept or not.  On the white-noise inputs of these tests the spectrum is
          flat, so the L2 statement over the kept bins is the same fraction of the error as of the signal.

  rel_C   relative L2 error of a correlation map computed from two such spectra,
            rel_C = rel_S(cur) + rel_S(ref) + (sqrt(2) gamma_2 + u) + cols_inv + rows_inv
          (the conjugate product and the 1 / (H W) scale, then the inverse passes).  Per value
            E = CAP rel_C rms(cc64).

  arg-max   any implementation whose map is within E of cc64 pointwise returns p with cc64[p] >= max(cc64) - 2 E
            (its own value at p is at least its value at the true maximum).  No pair is excluded.
  nb        |nb - neighbourhood64(cc64, p)| <= E, NaN exactly where the definition has NaN -- for the row transform
            of mc_xc_peak_neighbourhood and for the nine direct sums of mc_xcg_peak_neighbourhood alike.
  parabola  off = (v0 - v2) / (2 den), den = v0 - 2 v1 + v2.  First order in errors |dv_i| <= E:
            d off = (dv0 - dv2) / (2 den) - off d den / den, |dv0 - dv2| <= 2E, |d den| <= 4E, so
            |d off| <= (E + 4 E |off|) / |den|; with the denominator itself known only to 4E:
            |off - off64| <= E (1 + 4 |off64|) / (|den64| - 4E)   (no statement when |den64| <= 4E).
  accumulate   mc_field_accumulate from GIVEN peaks and neighbourhoods, with the pixel spacing and the threshold at
            the fp32 values the kernel receives, is a fixed chain of eight single fp32 roundings per value:
            (1) n = v0 - v2, (2) a = v0 - 2 v1, (3) den = a + v2, (4) q = (n / 2) / den, (5) f = i + q,
            (6) s = f - P when the position wraps, (7) s * pixel_spacing, (8) field + that (2 v1 and n / 2 are exact).
            (1) and (4) are u |q| each; (2) and (3) are u |a| and u |den| of the denominator, i.e. amp u |q| with
            amp = (|a| + |den|) / |den|; (5) is u |f|, (6) u |s|.  A rejected patch gets the mean of the accepted
            shifts, formed in float64 from fp32 values and rounded once: the largest error among the accepted plus
            u |mean|.  accumulate64 returns the sum per entry,
              bound = ps ((2 + amp) u |q| + u |f| + u |s|) + u |s ps| + u |field|,
            and that, with nothing added, is what the test uses.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

import fourier_reference as fr
from global_refine_reference import filtered_spectra, parabola_offset, wrap  # noqa: F401  (re-exported)
from oracle import motion as om

U, ETA, C_MUL, GAMMA, CAP = fr.U, fr.ETA, fr.C_MUL, fr.GAMMA, fr.CAP
F32 = np.float32
MAX_TIES = 4  # noise and near-tie pairs: at most this many positions of the float64 map within 2E of its maximum


# ------------------------------------------------------------------ geometry and tables


def geometry(plan_args):
    """The pruning geometry the engine's plan has for `plan_args` = (h, w, pixel_spacing, b_factor,
    frequency_range): host arithmetic of plan.xc_geometry only."""
    from torch_motion_correction_amd import plan

    h, w, ps, _, fr_ = plan_args
    _, high = plan.band_limits(fr_, ps)
    return plan.xc_geometry(h, w, high, min(h, w) / 4, min(h, w) / 8)


def kept_rows(g):
    return np.concatenate([np.arange(g.kyp), np.arange(g.H - g.kyn, g.H)]).astype(np.int64)


def _key(plan_args):
    h, w, ps, b, fr_ = plan_args
    return int(h), int(w), float(ps), float(b), tuple(float(v) for v in fr_)


@functools.lru_cache(maxsize=8)
def _tables(key):
    h, w, ps, b, fr_ = key
    mask, benv, band = om._filters((h, w), ps, b, fr_)
    g = geometry(key)
    full = (band.double() * benv.double()).numpy()  # (h, w//2+1)
    filt = np.ascontiguousarray(full[kept_rows(g)][:, :g.nkx].T)  # (nkx, nky)
    outside = full.copy()
    outside[kept_rows(g)[:, None], np.arange(g.nkx)[None, :]] = 0.0
    assert not outside.any(), "the plan prunes a bin the filter keeps"
    fy = np.fft.fftfreq(h)[kept_rows(g)][None, :]
    fx = (np.arange(g.nkx) / w)[:, None]
    expo = float((b * (fy ** 2 + fx ** 2) / (4 * ps * ps) * (filt != 0)).max())
    return mask.double().numpy(), filt, expo


def tables64(plan_args):
    """(mask (h, w), filt (nkx, nky), largest exponent |E| of the envelope on a kept bin), float64."""
    return _tables(_key(plan_args))


def _frames64(frames):
    if isinstance(frames, torch.Tensor):
        return frames.detach().cpu().to(torch.float64).numpy()
    return np.asarray(frames, dtype=np.float64)


def box_stats64(frames):
    """(mean, unbiased std) of the central box over all frames jointly (normalize_image), float64."""
    x = _frames64(frames)
    _, h, w = x.shape
    box = x[:, int(0.25 * h):int(0.75 * h), int(0.25 * w):int(0.75 * w)]
    return float(box.mean()), float(box.std(ddof=1))


# ------------------------------------------------------------------ the definitions


def spectra_parts(frames, plan_args, jobs=None, expo=None, stats=None):
    """The filtered spectra of `jobs` and what the bounds need of them.  `frames` (t, H, W) of any real dtype, taken
    at its float64 value; `plan_args` = (h, w, pixel_spacing, b_factor, frequency_range) of the WINDOW; `jobs` a list
    of (frame, y0, x0) window origins (None: every whole frame); `expo` the per-job mask exponent (None: 1);
    `stats` = (mean, std) to normalise with (None: box_stats64 of the frames).
    -> dict: S (njobs, nkx, nky) complex128, filt (nkx, nky), rms (njobs,) the rms of each job's UNFILTERED full
    spectrum (= ||x_n mask^e||_2), mean, std."""
    x = _frames64(frames)
    h, w = int(plan_args[0]), int(plan_args[1])
    mask, filt, _ = tables64(plan_args)
    g = geometry(plan_args)
    rows = kept_rows(g)
    mean, std = box_stats64(x) if stats is None else (float(stats[0]), float(stats[1]))
    if jobs is None:
        assert x.shape[1:] == (h, w), (x.shape, plan_args)
        jobs = [(f, 0, 0) for f in range(x.shape[0])]
    expo = [1] * len(jobs) if expo is None else [int(e) for e in expo]
    S = np.empty((len(jobs), g.nkx, len(rows)), dtype=np.complex128)
    rms = np.empty(len(jobs))
    for j, ((f, y0, x0), e) in enumerate(zip(jobs, expo)):
        xn = (x[f, y0:y0 + h, x0:x0 + w] - mean) / std * mask ** e
        rms[j] = np.linalg.norm(xn)
        S[j] = np.fft.rfft2(xn)[rows][:, :g.nkx].T * filt
    return {"S": S, "filt": filt, "rms": rms, "mean": mean, "std": std}


def spectra64(frames, plan_args, jobs=None, expo=None, stats=None):
    """(njobs, nkx, nky) complex128: rfft2((x - mean) / std * mask^e) * band * envelope on the kept bins, laid out
    as engine._forward_spectra writes it (kept columns first, then the kept rows: ky < kyp, then the last kyn)."""
    return spectra_parts(frames, plan_args, jobs, expo, stats)["S"]


def full_spectrum(S, plan_args):
    """The (H, W//2+1) rfft2 layout of one pruned spectrum (nkx, nky): zeros on every bin that is not kept."""
    g = geometry(plan_args)
    out = np.zeros((g.H, g.W // 2 + 1), dtype=np.complex128)
    out[kept_rows(g)[:, None], np.arange(g.nkx)[None, :]] = np.asarray(S).T
    return out


def correlation64(S_cur, S_ref, plan_args):
    """irfft2(conj(ref) cur, s=(H, W)) of two pruned spectra: the full (H, W) map with the kernels' 1 / (H W)
    scale (numpy's irfft2 applies it)."""
    g = geometry(plan_args)
    return np.fft.irfft2(np.conj(full_spectrum(S_ref, plan_args)) * full_spectrum(S_cur, plan_args), s=(g.H, g.W))


def neighbourhood64(cc, peak):
    """(3, 3) values of the map at (py - 1 .. py + 1, px - 1 .. px + 1), NaN outside the map: the rule of
    mc_xc_peak_neighbourhood -- NOT circular."""
    h, w = cc.shape
    py, px = divmod(int(peak), w)
    nb = np.full((3, 3), np.nan)
    for i in range(3):
        for j in range(3):
            y, x = py + i - 1, px + j - 1
            if 0 <= y < h and 0 <= x < w:
                nb[i, j] = cc[y, x]
    return nb


def offsets64(nb):
    """(oy, ox) of the reference's parabola (estimate_motion_xc.py:465-481, its `!=` guards) from a (3, 3)
    neighbourhood: the column through the centre for y, the row for x; none at all when any of the four outer
    samples is missing (a peak on the border, rule Q4)."""
    nb = np.asarray(nb, dtype=np.float64)
    if np.isnan(nb[[0, 2, 1, 1], [1, 1, 0, 2]]).any():
        return 0.0, 0.0
    return parabola_offset(nb[0, 1], nb[1, 1], nb[2, 1]), parabola_offset(nb[1, 0], nb[1, 1], nb[1, 2])


def shifts64(peak, shape):
    py, px = divmod(int(peak), shape[1])
    return wrap(py, shape[0]), wrap(px, shape[1])


def accumulate64(peaks, nb, frames, npatch, P, t, pixel_spacing, threshold, flags, field0=None):
    """mc_field_accumulate's documented contract (include/mcorr.h) in float64, from given peaks (nf * npatch,) and
    neighbourhoods (nf * npatch, 3, 3): pair p = fi * npatch + g belongs to frame frames[fi]; position = peak +
    parabola offsets when flags & 1 and the peak is not on the border; wrap-around `v if v <= P // 2 else v - P` of
    the (fractional) position; when flags & 2 (and npatch > 1) the outlier rejection of estimate_motion_xc.py:538-627
    (z = |s - lower median| / max(unbiased std, 1e-6) per axis, either axis beyond the threshold replaces both by the
    mean of the accepted patches, the median when none is accepted); field[c, frame, g] += shift * pixel_spacing.
    `pixel_spacing` and `threshold` are taken at their fp32 values, as the kernel receives them.
    -> (field (2, t, npatch) float64, bound (2, t, npatch): the eight roundings of the module docstring, per entry)."""
    peaks = np.asarray(peaks, dtype=np.int64)
    ps, thr = float(np.float32(pixel_spacing)), float(np.float32(threshold))
    nf = len(frames)
    field = np.zeros((2, t, npatch)) if field0 is None else np.array(field0, dtype=np.float64).reshape(2, t, npatch)
    bound = np.zeros((2, t, npatch))
    for fi in range(nf):
        s, err = np.zeros((2, npatch)), np.zeros((2, npatch))
        for g in range(npatch):
            p = fi * npatch + g
            iy, ix = divmod(int(peaks[p]), P)
            pos, e = [float(iy), float(ix)], [0.0, 0.0]
            if flags & 1 and 1 <= iy < P - 1 and 1 <= ix < P - 1:
                q = np.asarray(nb[p], dtype=np.float64)
                for c, (v0, v1, v2) in enumerate(((q[0, 1], q[1, 1], q[2, 1]), (q[1, 0], q[1, 1], q[1, 2]))):
                    if v2 != v0:  # NaN outer samples compare unequal and give NaN, as the kernel's float compare
                        a = v0 - 2 * v1
                        den = a + v2
                        off = 0.5 * (v0 - v2) / den
                        amp = (abs(a) + abs(den)) / abs(den) if den else np.inf
                        pos[c] += off
                        e[c] = (2 + amp) * U * abs(off) + U * abs(pos[c])  # roundings (1) - (5)
            for c in range(2):
                wrapped = pos[c] > P // 2
                s[c, g] = pos[c] - P if wrapped else pos[c]
                err[c, g] = e[c] + (U * abs(s[c, g]) if wrapped else 0.0)  # (6)
        if flags & 2 and npatch > 1:
            med = np.sort(s, axis=1)[:, (npatch - 1) // 2]
            sd = np.maximum(s.std(axis=1, ddof=1), 1e-6)
            bad = (np.abs(s - med[:, None]) / sd[:, None] > thr).any(axis=0)
            ok = ~bad
            rep = s[:, ok].mean(axis=1) if ok.any() else med
            rep_err = (err[:, ok].max(axis=1) if ok.any() else err.max(axis=1)) + U * np.abs(rep)
            s[:, bad] = rep[:, None]
            err[:, bad] = rep_err[:, None]
        val = s * ps
        new = field[:, frames[fi], :] + val
        bound[:, frames[fi], :] = ps * err + U * np.abs(val) + U * np.abs(new)  # (7), (8)
        field[:, frames[fi], :] = new
    return field, bound


# ------------------------------------------------------------------ the bounds


def line_costs(g):
    """Relative L2 error of each of the four 1-D passes of the pruned engine for geometry `g`, and the kind of line
    that runs it, taken from the plan as fourier_reference.transform_cost takes them."""
    from torch_motion_correction_amd import plan

    w, h = int(g.W), int(g.H)
    pack = ETA if w % 2 == 0 else 0.0
    n_r = plan.row_line_length(w)
    kinds = {}
    if plan.native_rows(g):
        rf = ri = fr._fft_cost(n_r) + pack
        kinds["rows"] = "native"
    else:
        rf, kf = fr._line_cost(n_r, -1, plan.row_line_keep(w, g.nkx))
        ri, ki = fr._line_cost(n_r, +1)
        rf, ri, kinds["rows"] = rf + pack, ri + pack, f"{kf} / {ki}" if kf != ki else ki
    if plan.native_height(h):
        cf = ci = fr._fft_cost(h)
        kinds["cols"] = "native"
    else:
        cf, _ = fr._line_cost(h, -1)
        ci, kinds["cols"] = fr._line_cost(h, +1)
    return {"rows_fwd": rf, "cols_fwd": cf, "rows_inv": ri, "cols_inv": ci, "kinds": kinds}


def spectra_bounds(plan_args, mean, std, expo=1, conditioning=0.0, fused=None):
    """rel_S of one job and its named terms (module docstring).  `expo`: the job's mask exponent; `conditioning`:
    ||conditioning_error||_2 / ||conditioned job||_2 for raw input; `fused` = (d, Mhat64 (nkx, nky)) for the
    fused-statistics route, d = |mean - m0| / std.  -> dict with 'rel', 'fix_l2' (absolute), 'fix_bin' (nkx, nky)
    (absolute, already times CAP) and the terms."""
    mask, filt, emax = tables64(plan_args)
    g = geometry(plan_args)
    lc = line_costs(g)
    norm = (5 + abs(mean) / std) * U
    ring = np.count_nonzero((mask > 0) & (mask < 1))
    mterm = expo * 6 * U * math.sqrt(ring / float((mask ** (2 * expo)).sum())) + expo * U
    fterm = U + 2 * (10 * emax + 2) * U
    fft = lc["rows_fwd"] + lc["cols_fwd"]
    rel = norm + mterm + fft + fterm + conditioning
    out = {"norm": norm, "mask": mterm, "fft": fft, "filter": fterm, "conditioning": conditioning, "kinds": lc["kinds"],
           "fix_l2": 0.0, "fix_bin": 0.0}
    if fused is not None:
        d, mhat = fused
        rel = norm + mterm + fft * math.sqrt(1 + d * d) + fterm + conditioning
        fm = np.abs(filt * mhat)
        out["fix_l2"] = d * (fft + 2 * U) * float(np.linalg.norm(fm))
        out["fix_bin"] = d * (fft + 2 * U) * CAP * fm
        out["d"] = d
    out["rel"] = rel
    return out


def mask_spectrum64(plan_args):
    """Mhat of the fused-statistics route: the unfiltered pruned spectrum of the mask itself, (nkx, nky)."""
    mask, _, _ = tables64(plan_args)
    g = geometry(plan_args)
    return np.fft.rfft2(mask)[kept_rows(g)][:, :g.nkx].T


def map_bounds(plan_args, rel_cur, rel_ref, cc64):
    """(rel_C, E) of one pair's map (module docstring)."""
    lc = line_costs(geometry(plan_args))
    rel_c = rel_cur + rel_ref + math.sqrt(2) * GAMMA(2) + U + lc["cols_inv"] + lc["rows_inv"]
    return rel_c, CAP * rel_c * float(np.sqrt(np.mean(np.square(cc64))))


def parabola_bound(v0, v1, v2, E):
    """|off - off64| <= E (1 + 4 |off64|) / (|den64| - 4 E); inf when the denominator is not known to 4E."""
    den = v0 - 2 * v1 + v2
    if abs(den) <= 4 * E:
        return math.inf
    return E * (1 + 4 * abs(parabola_offset(v0, v1, v2))) / (abs(den) - 4 * E)


# ------------------------------------------------------------------ the comparisons (shared by host and GPU tests)


def as_complex(S):
    """A (.., 2) fp32 tensor of the engine, or a complex array, as complex128 numpy."""
    if isinstance(S, torch.Tensor):
        S = S.detach().cpu()
        if not S.is_complex():
            S = torch.view_as_complex(S.double().contiguous())
        return S.to(torch.complex128).numpy()
    return np.asarray(S, dtype=np.complex128)


def check_spectra(got, parts, bounds, what):
    """Every job of `got` (njobs, nkx, nky) against parts['S']: finite, exact zeros where the filter is zero, L2
    within rel ||S64|| + fix_l2, every other bin within CAP rel filt[bin] rms + fix_bin.  `bounds`: one
    spectra_bounds dict, or one per job.  -> (worst L2 ratio, worst per-bin ratio); raises AssertionError."""
    got = as_complex(got)
    ref, filt = parts["S"], parts["filt"]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got.view(np.float64)).all(), f"{what}: non-finite spectrum"
    zero = filt == 0
    worst_l2 = worst_bin = 0.0
    for j in range(ref.shape[0]):
        b = bounds[j] if isinstance(bounds, (list, tuple)) else bounds
        nz = int(np.count_nonzero(got[j][zero]))
        assert nz == 0, f"{what} job {j}: {nz} filtered-out bins are not exactly zero"
        d = np.abs(got[j] - ref[j])
        l2, norm = float(np.linalg.norm(d)), float(np.linalg.norm(ref[j]))
        l2_bound = b["rel"] * norm + b["fix_l2"]
        cap = CAP * b["rel"] * filt * parts["rms"][j] + b["fix_bin"]
        ratio = np.where(zero, 0.0, d / np.where(zero, 1.0, cap))
        k = int(np.argmax(ratio))
        print(f"  {what} job {j}: L2 {l2 / norm:.3e} bound {l2_bound / norm:.3e}; worst bin {ratio.flat[k]:.3f} of its cap "
              f"at {np.unravel_index(k, ratio.shape)}")
        assert l2 <= l2_bound, f"{what} job {j}: relative L2 {l2 / norm:.3e} > {l2_bound / norm:.3e}"
        assert ratio.flat[k] <= 1.0, (f"{what} job {j}: bin {np.unravel_index(k, ratio.shape)} off by {d.flat[k]:.3e} > "
                                      f"{cap.flat[k]:.3e}")
        worst_l2, worst_bin = max(worst_l2, l2 / l2_bound), max(worst_bin, float(ratio.flat[k]))
    return worst_l2, worst_bin


def check_map(got, cc64, rel_c, E, what):
    """A full map against cc64: L2 within rel_C, every value within E.  -> (L2 ratio, value ratio)."""
    l2, mx, _ = fr.measure(np.asarray(got, dtype=np.float64), cc64)
    norm = float(np.linalg.norm(cc64))
    print(f"  {what}: map L2 {l2 / norm:.3e} bound {rel_c:.3e}; max {mx:.3e} E {E:.3e}")
    assert l2 <= rel_c * norm, f"{what}: map relative L2 {l2 / norm:.3e} > {rel_c:.3e}"
    assert mx <= E, f"{what}: map value off by {mx:.3e} > {E:.3e}"
    return l2 / (rel_c * norm), mx / E


def admissible(cc64, E):
    """Flat indices of the map within 2E of its maximum."""
    flat = cc64.reshape(-1)
    return np.nonzero(flat >= flat.max() - 2 * E)[0]


def check_peak(peak, shift, cc64, E, what):
    """The arg-max criterion: a valid index with cc64[p] >= max - 2E, and `shift` (None to leave out) exactly the
    wrapped index.  -> (max - cc64[p]) / 2E."""
    h, w = cc64.shape
    p = int(peak)
    assert 0 <= p < h * w, f"{what}: peak {p} is not an index of a {h} x {w} map"
    top = float(cc64.max())
    val = float(cc64.reshape(-1)[p])
    print(f"  {what}: peak {divmod(p, w)} value {val:.6e} max {top:.6e} 2E {2 * E:.3e}")
    assert val >= top - 2 * E, f"{what}: peak {divmod(p, w)} has {val:.6e} < max {top:.6e} - 2E ({2 * E:.3e})"
    if shift is not None:
        want = shifts64(p, (h, w))
        assert (float(shift[0]), float(shift[1])) == (float(want[0]), float(want[1])), f"{what}: shift {shift} != {want}"
    return (top - val) / (2 * E)


def check_neighbourhood(nb, cc64, peak, E, what):
    """|nb - neighbourhood64| <= E elementwise, NaN exactly where the definition has NaN.  -> ratio."""
    nb = np.asarray(nb, dtype=np.float64).reshape(3, 3)
    ref = neighbourhood64(cc64, peak)
    assert np.array_equal(np.isnan(nb), np.isnan(ref)), f"{what}: NaN pattern {np.isnan(nb).tolist()} != {np.isnan(ref).tolist()}"
    tol = np.full((3, 3), float(E))
    ok = ~np.isnan(ref)
    ratio = float((np.abs(nb - ref)[ok] / tol[ok]).max()) if ok.any() else 0.0
    print(f"  {what}: neighbourhood worst {ratio:.3f} of E")
    assert ratio <= 1.0, f"{what}: neighbourhood off by {ratio:.3f} E:\n{nb}\n{ref}"
    return ratio


def check_offsets(nb, cc64, peak, E, what):
    """offsets64 of `nb` against offsets64 of the float64 neighbourhood, each axis within parabola_bound; the bound
    holds across the `!=` guard (its 0 is the continuous limit of (v0 - v2) / (2 den)).  Only an axis whose float64
    denominator is within 4E of zero has no statement beyond a finite offset.  -> worst ratio."""
    ref = neighbourhood64(cc64, peak)
    got, want = offsets64(nb), offsets64(ref)
    if np.isnan(ref[[0, 2, 1, 1], [1, 1, 0, 2]]).any():
        assert got == (0.0, 0.0), f"{what}: offsets {got} for a peak on the border"
        return 0.0
    worst = 0.0
    for c, (v0, v1, v2) in enumerate(((ref[0, 1], ref[1, 1], ref[2, 1]), (ref[1, 0], ref[1, 1], ref[1, 2]))):
        b = parabola_bound(v0, v1, v2, E)
        assert math.isfinite(got[c]), f"{what}: axis {c} offset {got[c]}"
        if not math.isfinite(b):
            continue
        print(f"  {what}: axis {c} offset {got[c]:+.6f} float64 {want[c]:+.6f} bound {b:.3e}")
        assert abs(got[c] - want[c]) <= b, f"{what}: axis {c} offset {got[c]} vs {want[c]}, bound {b:.3e}"
        worst = max(worst, abs(got[c] - want[c]) / b)
    return worst


# ------------------------------------------------------------------ inputs and case tables

DEFAULT_BAND = (300.0, 10.0)
B_FACTOR = 500.0


def args(h, w, ps=1.0, band=DEFAULT_BAND):
    return (h, w, float(ps), B_FACTOR, tuple(band))


def noise(t, h, w, mean=0.0, std=1.0, seed=0):
    """White noise N(mean, std^2), fp32 (t, h, w)."""
    g = torch.Generator().manual_seed(seed * 100003 + t * 7919 + h * 31 + w)
    return torch.randn(t, h, w, generator=g) * std + mean


def planted(t, h, w, shifts, seed=0, noise_sigma=0.5):
    """A periodic white-noise texture rolled by `shifts` ((t, 2) integers; frame f shows it displaced by +shift[f]),
    plus fresh white noise: the correlation of frame f with frame r peaks at shift[f] - shift[r] (mod the frame)."""
    g = torch.Generator().manual_seed(seed * 100003 + t * 7919 + h * 31 + w + 1)
    base = torch.randn(h, w, generator=g)
    return torch.stack([torch.roll(base, (int(sy), int(sx)), (0, 1)) + noise_sigma * torch.randn(h, w, generator=g)
                        for sy, sx in shifts])


# forward spectra on small shapes (host: the fp32 oracle inside the bounds; GPU: the kernels): (t, h, w, ps, band)
SPECTRA_SMALL = [(3, 64, 64, 1.0, DEFAULT_BAND), (2, 256, 256, 0.83, DEFAULT_BAND), (2, 256, 256, 2.5, DEFAULT_BAND),
                 (2, 256, 512, 1.0, DEFAULT_BAND), (2, 512, 256, 2.5, DEFAULT_BAND), (3, 100, 120, 1.0, DEFAULT_BAND),
                 (2, 64, 1440, 1.0, DEFAULT_BAND), (2, 121, 128, 1.0, DEFAULT_BAND), (2, 121, 135, 1.0, DEFAULT_BAND)]
# rows of 4096 columns and tall columns: (t, h, w, ps, band)
SPECTRA_WIDE = [(2, 512, 4096, 1.0, DEFAULT_BAND), (2, 512, 4096, 1.0, (300.0, 20.0)), (2, 1024, 4096, 1.0, DEFAULT_BAND),
                (2, 1024, 4096, 1.0, (300.0, 20.0)), (2, 4096, 256, 1.0, DEFAULT_BAND), (2, 1024, 256, 1.0, DEFAULT_BAND)]
# direct mixed-radix and long chirp-z lines: (t, h, w, ps, band).  (2, 4100, 128) was meant to reach the chirp-z length
# 16384; 2 * 4100 - 1 = 8199 fits 10240, so its columns run M = 10240 -- it stays, asserted as what it is -- and
# (2, 5200, 128) (2 * 5200 - 1 = 10399 > 10240) is the case that runs M = 16384.
SPECTRA_LINES = [(2, 96, 5760, 1.0, DEFAULT_BAND), (2, 2880, 128, 1.0, DEFAULT_BAND), (2, 96, 7000, 1.0, DEFAULT_BAND),
                 (2, 4100, 128, 1.0, DEFAULT_BAND), (2, 5200, 128, 1.0, DEFAULT_BAND)]
WIDE_BAND = (2, 256, 4096, 1.0, (300.0, 3.0))  # nkx > 512: the general kernels on 4096-column rows
BENCH = (3, 4096, 4096, 1.0, DEFAULT_BAND)
STAT_INPUTS = [(0.0, 1.0), (40.0, 2.5), (1000.0, 30.0)]
# map / arg-max / neighbourhood: (t, h, w)
MAP_SEPARATE = [(5, 256, 256), (4, 512, 512), (3, 100, 120), (2, 121, 135), (2, 96, 5760)]
MAP_FUSED = [(6, 1024, 1024), (3, 4096, 256)]


# ------------------------------------------------------------------ raw patch jobs (mc_xc_rows_forward_dual_raw)
# One input for tests/test_xc_kernels_float64.py (the kernel) and tests/test_xc_reference_host.py (the fp32
# restatement and the planted faults), so that the two cannot drift apart.

RAW_PATCH_MARGIN = (9, 15)  # frames are (h + 9, 1024 + 15): an ODD width (1039), so row starts alternate in parity
# (frame, y0, x0), not sorted by frame: x0 odd (13, 3, 15), x0 % 4 == 2 (6), y0 * W + x0 odd ((9, 6), (4, 15)), and the
# origin of frame 1, whose offset is a whole frame: job_off % frame_area == 0 with job_off != 0
RAW_PATCH_JOBS = [(1, 7, 13), (0, 1, 3), (1, 0, 0), (0, 9, 6), (1, 4, 15)]
RAW_PATCH_EXPO = ((1, 2, 3, 1, 1), (2, 4, 6, 2, 2))  # the (1, 2) pair of the fast path and the power loops in one launch
RAW_PATCH_HEIGHTS = (1024, 16)  # windows (h, 1024): ny = 800 (ny % 32 == 0) and ny = 16 (the group tail, ny % 32 != 0)
RAW_KINDS = {"u8": torch.uint8, "i16": torch.int16}


def raw_patch_frame(h):
    return h + RAW_PATCH_MARGIN[0], 1024 + RAW_PATCH_MARGIN[1]


def raw_patch_offsets(h, jobs=RAW_PATCH_JOBS):
    H, W = raw_patch_frame(h)
    return [f * H * W + y0 * W + x0 for f, y0, x0 in jobs]


def check_raw_patch_jobs(h, jobs=RAW_PATCH_JOBS):
    """The properties the job list is there for (asserted, not assumed)."""
    H, W = raw_patch_frame(h)
    off = raw_patch_offsets(h, jobs)
    frames = [f for f, _, _ in jobs]
    assert len(jobs) >= 5 and set(frames) == {0, 1} and frames != sorted(frames), jobs
    assert all(0 <= y0 <= H - h and 0 <= x0 <= W - 1024 for _, y0, x0 in jobs), "a window leaves its frame"
    assert W % 2 == 1 and (H * W) % 2 == 1
    assert any(x0 % 2 == 1 for _, _, x0 in jobs) and any(x0 % 4 == 2 for _, _, x0 in jobs)
    assert any((y0 * W + x0) % 2 == 1 for _, y0, x0 in jobs)
    assert any(o != 0 and o % (H * W) == 0 for o in off), "no job at the origin of frame 1"
    assert {o % 2 for o in off} == {0, 1} and any(o % 4 == 2 for o in off)
    return off


@functools.lru_cache(maxsize=4)
def raw_patch_input(kind, h=1024):
    """-> (raw (2, H, W) u8 / i16, gain (H, W) fp32) of the raw patch tests.  Counts: kernel_harness.drifting_raw_movie
    (a texture in [10, 50) + noise), frame 1 drifted and BRIGHTER -- u8 by 12 counts of a mean of 30; i16 (8 v - 340
    against 8 v - 240: means of about -100 and 0, a difference as large as the mean) -- so that a job that takes the
    other frame's subtrahend is off by a constant of more than a quarter of a standard deviation, over ten thousand
    times the bound (with a gain of this range the conditioned standard deviation is itself three quarters of the
    brightness, so the difference cannot be many standard deviations; what counts is its size against the bound,
    and both are asserted by the tests).  i16: four fifths of frame 0 and half of frame 1 are negative.  Gain: kernel_harness.gain, log-uniform
    in [0.25, 4]."""
    import kernel_harness as kh

    H, W = raw_patch_frame(h)
    dtype = RAW_KINDS[kind]
    raw = kh.drifting_raw_movie([0, 3], [0, -2], H, W, dtype, seed=41 + h + (kind == "u8"))
    if kind == "u8":
        raw[1] += 12
        assert int(raw.max()) < 250
    else:
        raw -= torch.tensor([240, 140], dtype=torch.int16)[:, None, None]
        assert float((raw < 0).float().mean()) >= 0.25
        for f, y0, x0 in RAW_PATCH_JOBS:  # negative counts in both halves of the pairs of every window
            neg = raw[f, y0:y0 + h, x0:x0 + 1024] < 0
            assert bool(neg[:, 0::2].any()) and bool(neg[:, 1::2].any()) and bool((neg[:, 0::2] & neg[:, 1::2]).any())
    m = raw.double().mean(dim=(1, 2))
    assert float(m[1] - m[0]) >= 0.25 * abs(float(m[0])), m
    return raw, kh.gain(H, W)


def raw_stats64(raw, gain):
    """(sub (t,) fp32, rstd fp32) of engine.RawMovie(raw, gain) by raw_stats_finalize's formulas on float64 moments:
    mu_f = fp32(frame mean of raw * gain), the mean and the unbiased std of raw * gain - mu_f over the central box of
    all frames jointly, sub_f = fp32(mu_f + fp32(mean)), rstd = fp32(1 / std).  For the host tests, which have no
    device to ask."""
    x = raw.double().numpy() * gain.double().numpy()
    _, H, W = x.shape
    mu = x.mean(axis=(1, 2)).astype(F32)
    c = (x - mu.astype(np.float64)[:, None, None])[:, int(0.25 * H):int(0.75 * H), int(0.25 * W):int(0.75 * W)]
    return (mu + F32(c.mean())).astype(F32), F32(1.0 / c.std(ddof=1))


@functools.lru_cache(maxsize=8)
def _raw_patch_reference(kind, plan_args, sub, rstd, expo):
    from rigid_reference import condition_float64, conditioning_error

    h = int(plan_args[0])
    raw, gain = raw_patch_input(kind, h)
    sub = np.asarray(sub, dtype=F32)
    std = 1.0 / float(rstd)
    v = condition_float64(raw.numpy(), gain.numpy(), sub)
    parts = spectra_parts(v, plan_args, RAW_PATCH_JOBS, expo, stats=(0.0, std))
    mask = tables64(plan_args)[0]
    bounds = []
    for (f, y0, x0), e in zip(RAW_PATCH_JOBS, expo):
        win = (slice(y0, y0 + h), slice(x0, x0 + 1024))
        err = conditioning_error(raw[f][win].numpy(), gain[win].numpy(), sub[f])
        c = float(np.linalg.norm(err * mask ** e) / np.linalg.norm(v[f][win] * mask ** e))
        bounds.append(spectra_bounds(plan_args, 0.0, std, expo=e, conditioning=c))
    return parts, bounds


def raw_patch_reference(kind, plan_args, sub, rstd, expo):
    """(parts, [bounds per job]) of RAW_PATCH_JOBS with the mask exponents `expo` on raw_patch_input(kind, h): the
    float64 conditioning (raw * gain - sub_f) with the subtrahends and 1 / std the kernels were given, spectra_parts
    with stats (0, 1 / rstd), and per job spectra_bounds with the conditioning term
    ||conditioning_error mask^e||_2 / ||v mask^e||_2 over that job's window.  Computed once per argument set."""
    return _raw_patch_reference(kind, _key(plan_args), tuple(float(s) for s in sub), float(rstd),
                                tuple(int(e) for e in expo))


def point_symmetric(x):
    """x + its point reflection about the mask centre (h // 2, w // 2), indices taken circularly: exactly symmetric
    in fp32 (a sum of two floats commutes)."""
    h, w = x.shape
    iy = (2 * (h // 2) - torch.arange(h)) % h
    ix = (2 * (w // 2) - torch.arange(w)) % w
    return x + x[iy][:, ix]


TIE_SHIFTS = [(3, -5), (7, 2), (-4, 6), (0, 9), (5, 0), (6, 6)]


def tied(t, h, w, seed=7):
    """Near-tie input: the reference frame t // 2 is a point-symmetric texture B (about the centre of the equally
    symmetric mask), every other frame holds two equal-weight copies of it, roll(B, +s) + roll(B, -s), which is
    point-symmetric again.  The correlation map then satisfies cc(d) = cc(-d) exactly, so its maximum is attained
    twice, at +s and -s: in float64 the two values differ by rounding only, far less than 2E, and an fp32 map may
    pick either.  This is the tolerant branch of the arg-max criterion; white noise almost never ties within 2E."""
    g = torch.Generator().manual_seed(seed * 100003 + t * 7919 + h * 31 + w)
    base = point_symmetric(torch.randn(h, w, generator=g))
    frames = [torch.roll(base, TIE_SHIFTS[f % len(TIE_SHIFTS)], (0, 1)) + torch.roll(base, tuple(-v for v in TIE_SHIFTS[f % len(TIE_SHIFTS)]), (0, 1))
              for f in range(t)]
    frames[t // 2] = base
    return torch.stack(frames)


def small_drift(t):
    return [(int(round(-6 + 14 * f / max(t - 1, 1))), int(round(5 - 9 * f / max(t - 1, 1)))) for f in range(t)]


def large_drift(t, h, w):
    """Shifts of a quarter of the shorter side -- as far as the soft disk mask (radius 1/4, edge to 3/8 of it) leaves
    the two frames a common support worth a peak -- on one axis at a time and on both, both signs on both axes
    (relative to frame t // 2 = (0, 0)): 256 px on 1024 x 1024 frames."""
    a, c = min(h, w) // 4, min(h, w) // 32
    rows = [(a, -c), (-a, c), (c, a), (-c, -a), (a // 2, a // 2), (-a // 2, -a // 2)]
    out = [rows[f % len(rows)] for f in range(t)]
    out[t // 2] = (0, 0)
    return out


@functools.lru_cache(maxsize=4)
def map_reference(t, h, w, kind, near=None):
    """(movie fp32, plan_args, parts, [(f, cc64, rel_C, E) for every frame f != t // 2 against t // 2]) for one input
    kind of the map tables: 'small', 'large', 'noise', 'tie' (tied), 'border' (peaks on row 0 / column 0 / last row / last
    column), 'near' (`near` = mc_xc_near_rows: peaks in rows near - 9 and near - 8, the last searched row and the first
    beyond it when 8 of the stored rows are guard rows, their mirror images at the far end, and in rows near - 1 and
    near, the last stored row and the first that is not).  Computed once per case."""
    ref = t // 2
    if kind == "small":
        x = planted(t, h, w, small_drift(t))
    elif kind == "large":
        x = planted(t, h, w, large_drift(t, h, w))
    elif kind == "noise":
        x = noise(t, h, w, seed=17)
    elif kind == "tie":
        x = tied(t, h, w)
    elif kind == "border":
        rows = [(0, 5), (-1, 3), (4, 0), (2, -1), (0, 0), (-1, -1)]
        s = [rows[f % len(rows)] for f in range(t)]
        s[ref] = (0, 0)
        x = planted(t, h, w, s, seed=3)
    else:
        assert kind == "near" and near
        n = near - 8  # the header promises "searched rows plus a few guard rows": both readings of the edge are planted
        rows = [(n - 1, 3), (-n - 1, -3), (n, -2), (-n, 4), (near - 1, 0), (near, 1)]
        s = [rows[f % len(rows)] for f in range(t)]
        s[ref] = (0, 0)
        x = planted(t, h, w, s, seed=5)
    pa = args(h, w)
    parts = spectra_parts(x, pa)
    b = spectra_bounds(pa, parts["mean"], parts["std"])
    pairs = []
    for f in range(t):
        if f == ref:
            continue
        cc = correlation64(parts["S"][f], parts["S"][ref], pa)
        rel_c, E = map_bounds(pa, b["rel"], b["rel"], cc)
        pairs.append((f, cc, rel_c, E))
    return x, pa, parts, pairs
