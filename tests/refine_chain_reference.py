"""A derived float64 bound for the COMPOSED refinement iteration (refine_global_motion[_raw], refine_local_motion[_raw]):
mc_xc_aligned_refs[_patches] -> K3 / K4 / K6 -> mc_xc_refine_update[_patches], repeated ITER times, judged as a whole.

TEST INFRASTRUCTURE ONLY: numpy on the CPU.  Nothing here restates the arithmetic a third time.  The field a route is
held to is the restatement's -- global_refine_reference.refine_shifts for whole frames, local_refine_reference.
refine_patches per patch -- run on the float64 spectra of xc_reference.spectra_parts (the same definition as
filtered_spectra, on the kept bins; it also takes the float64 conditioning of raw counts).  The bound is composed of the
bounds the per-kernel files already derive, evaluated on float64 quantities alone; no constant comes from a GPU run.

THE BOUND, per case, per (frame, patch) and axis; u = 2^-24.

 Local error of iteration k, delta_k: what one iteration adds when it starts from the restatement's own shifts s_k.
  spectra   rel_S of every job: xc_reference.spectra_bounds of that plan (with the fused-statistics terms where both
            axes run native lines: the larger of the two statistics routes; with rigid_reference.conditioning_error in
            L2 for raw counts, as tests/test_xc_kernels_float64.py adds it; plus u |mu| per sample where the conditioned
            route's fp32 frame mean is formed on the device, one rounding of the float64 mean).
  G', REF   iteration_reference._aligned's per-bin bounds eG, eREF at s_k - o.  Two roundings that file leaves to its
            caller (it takes fy, fx as given): the engine forms the kept frequencies as fl(k fl(1 / n)), 2 u relative,
            which is 2 u |d| of the shift the ramp carries (handed over as d_err) and 2 pi 2 u c (|fy| + |fx|) |S| for
            the translate by c = refine_under_px.  In L2, relative:
              rel_cur_f = rel_S_f + ||eG_f|| / ||G'_f||
              rel_ref_f = (sum_{g != f} rel_S_g ||S_g|| / (t - 1) + ||eREF_f||) / ||REF_f||
            (the error of S enters REF linearly; ||REF_f|| is the norm of the float64 REF itself, cancellation included).
  map       xc_reference.map_bounds(rel_cur_f, rel_ref_f, cc64): E_f = CAP rel_C rms(cc64), cc64 = the restatement's map
            irfft2(conj(REF_f) G'_f) at iteration k.
  parabola  xc_reference.parabola_bound on the 3 x 3 values of cc64 at its own maximum:
            |off - off64| <= E (1 + 4 |off64|) / (|den64| - 4 E), per axis.
  update    iteration_reference.residuals64's rounding count e_r of the residual, then iteration_reference._recentre with
            e_r + parabola in place of e_r: damp (e_r + pb) + u |damp r| + u |s'| for the frame and for the reference
            frame, + u of the re-centred value.  One rounding that count leaves out because it takes damp at its fp32
            value: the restatement uses (t - 1) / t exactly, fl((t - 1) / t) is within u of it: u |damp r| more, for the
            frame and the reference frame.
  delta_k = that sum; delta_r_k = e_r + parabola bounds the residual itself.

 Propagation.  e_0 = 0 for the integer estimate (exact integers: a fitness condition below says it cannot flip); for a
 caller's whole-frame start, e_0 = |start64 - fl32(start64)| <= u |start|; for a patch start, which the engine
 resamples with mc_spline_lattice, 24 u |start|: post_reference section C evaluated at a knot (s = 0, p = (1, 0, 0, 0),
 so e_b = 4 u on the one unit weight of each of the three axes, 12 u, plus gamma_12 of the nested sums, 12 u).  Then, with |J_k| the elementwise absolute value of the Jacobian
 of ONE iteration of the restatement (shifts in, shifts out) at s_k,
              e_{k+1} = |J_k| e_k + delta_k          (a vector recursion: one entry per frame and axis)
              |max|r|_k - max|r64|_k| <= max (|R_k| e_k + delta_r_k),   R_k = d r / d s.
 J_k and R_k are central differences of the restatement in float64 with steps of 1e-3 and 1e-4 px; the two must agree to
 5 % in infinity norm (the linear regime), and the elementwise larger is used.  Columns that multiply an e_k entry of
 exactly 0 (the reference frame's row; everything at k = 0 after an integer start) are not differentiated.  Patches do
 not couple: the Jacobian is block-diagonal by patch (assert_patches_do_not_couple, once on the reference).

 Fitness conditions on the inputs (asserted by `fitness`, on float64 quantities alone; a case that fails one is given
 another input, never a skip): every parabola offset of every iteration <= 0.45; every residual inside the near
 window (-15, +47) px; each map's maximum is the only value within 2 E of it and its 3 x 3 neighbours lie inside the
 map with |den| > 4 E (so no frame or patch is excluded and no integer peak can flip); the two Jacobians agree (of the
 shifts and of the residuals, || |J(1e-3)| - |J(1e-4)| ||_inf <= 5 % of ||J||_inf); the composed per-kernel definitions
 end within 1e-9 px of the restatement (both are float64: a million times their own rounding, a million times below
 the bound); the field to refine exceeds 0.2 px somewhere (below that the integer estimate would already be within the
 planted fractions); the final bound <= 1e-4 px.

 REACH.  delta is dominated by the parabola term E / |den|, E = CAP rel_C rms(cc64): rel_C is fixed by the plan (some
 3e-5), so what an input can change is rms(cc64) / |den|, the flatness of the peak, which falls with the number of
 kept bins and with their frequency squared.  Both are set by the mask (a quarter of the side) and the band's upper
 edge in cycles / pixel.  64-px frames and 256-px patches meet 1e-4 px only with that edge at 0.5 cycles / pixel
 (5 A / px); 96-px patches do not meet it there (2.2e-4 px) but do at 10 A / px, every bin kept; 1024-px patches at the 0.12 cycles / pixel
 that the wave-per-row row pass needs (nkx <= 128) reach 2.8e-4 px.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import torch

import global_refine_reference as gr
import iteration_reference as ir
import local_refine_reference as lr
import xc_reference as xr
from rigid_reference import condition_float64, conditioning_error

U = ir.U
ITER = 3
STEPS = (1e-3, 1e-4)
J_AGREE = 0.05
MAX_OFFSET = 0.45
NEAR = (-15.0, 47.0)
FINAL = 1e-4  # px: tests/test_local_refine.py: "above 1e-4 px is a bug, not a tolerance"
SPLINE_ROUNDINGS = 24  # post_reference section C at a knot, see Propagation
RAW_KINDS = {"u8": torch.uint8, "i16": torch.int16}
PS = 2.5  # Angstrom per pixel: the 10 A edge of the default band lies at 0.25 cycles / pixel
BAND = (0.01, 0.25)  # cycles / pixel of the planted texture


def under_px(h, w):
    from torch_motion_correction_amd import engine

    return engine.refine_under_px(h, w)


# ------------------------------------------------------------------ the cases


class Case:
    """One input of the chain tests.  kind 'frame' / 'patch'; `p` the patch side; `ref` the reference frame (None:
    t // 2); `store` 'f32', 'f16', 'u8' or 'i16'; `start` 'integer' (whole frames: the engine's own integer estimate;
    patches: the rigid part rounded to whole pixels, as a (2, t, 1, 1) field) or 'caller' (the refined field off by
    (0.4, -0.3) px with alternating sign); `amp` the size of the planted whole-pixel drift."""

    def __init__(self, name, kind, shape, p=None, ref=None, store="f32", start="integer", amp=3, seed=0, ps=PS,
                 tex=BAND, noise=0.1, freq=xr.DEFAULT_BAND, frac=0.27):
        self.name, self.kind, self.shape, self.p, self.ref = name, kind, tuple(shape), p, ref
        self.store, self.start, self.amp, self.seed = store, start, amp, seed
        self.ps, self.tex, self.noise, self.freq, self.frac = float(ps), tuple(tex), noise, tuple(freq), frac

    def __repr__(self):
        return self.name


TINY = dict(ps=5.0, tex=(0.01, 0.45), noise=0.05)  # the 10 A edge at 0.5 cycles / pixel: the sharpest peak a mask of 16 px leaves
FRAME_CASES = [
    Case("4x64x64", "frame", (4, 64, 64), amp=1, **TINY),
    Case("2x64x64", "frame", (2, 64, 64), amp=1, **TINY),
    Case("65x64x64", "frame", (65, 64, 64), amp=1, **TINY),
    Case("5x256x256-ref0", "frame", (5, 256, 256), ref=0),
    Case("5x256x256-reflast", "frame", (5, 256, 256), ref=4),
    Case("3x100x120", "frame", (3, 100, 120), amp=1, **TINY),
    Case("3x121x135", "frame", (3, 121, 135), amp=1, **TINY),
    Case("3x1024x1024", "frame", (3, 1024, 1024)),
    Case("5x256x256-f16", "frame", (5, 256, 256), ref=0, store="f16"),
    # three frames: a start off by +-(0.4, -0.3) px then leaves residuals of 0.4, 0.8, 0.3 and 0.6 px, offsets <= 0.4
    Case("3x256x256-caller", "frame", (3, 256, 256), start="caller"),
]
PATCH_CASES = [
    # 96-px patches meet the limit only with every bin inside the band and next to no noise (9.99e-5 px)
    Case("4x200x240-p96", "patch", (4, 200, 240), p=96, amp=1, ps=10.0, tex=(0.01, 0.5), noise=0.01),
    Case("4x512x640-p256", "patch", (4, 512, 640), p=256, **TINY),
    Case("3x1537x1537-p1024", "patch", (3, 1537, 1537), p=1024),
    Case("3x300x320-p256-one", "patch", (3, 300, 320), p=256, amp=1, **TINY),
]
CHUNKED = Case("4x512x768-p256", "patch", (4, 512, 768), p=256, **TINY)  # 8 patches: chunks of 3, 3 and 2
RAW_CASES = [Case(f"3x1024x1024-{k}", "frame", (3, 1024, 1024), store=k) for k in RAW_KINDS] + \
            [Case(f"4x512x640-p256-{k}", "patch", (4, 512, 640), p=256, store=k, **TINY) for k in RAW_KINDS]
# NOT CASES, with the figure that keeps them out (the last fitness condition; see REACH in the module docstring):
# (3, 1537, 1537) with 1024-px patches at 1.2 A / px,
# the coarsest spacing whose plan keeps <= 128 columns and so takes the wave-per-row patch row pass, 2.8e-4 px.
CASES = {c.name: c for c in FRAME_CASES + PATCH_CASES + [CHUNKED] + RAW_CASES}
SMALL = ("4x64x64", "3x300x320-p256-one", "3x1537x1537-p1024")  # the stand-in and the planted faults run on these


def ref_frame(case):
    t = case.shape[0]
    return t // 2 if case.ref is None else case.ref % t


def planted_drifts(case):
    """(rigid (t, 2), slope (t, 2)): whole pixels up to `amp` plus fractions of at most 0.27 px (the leave-one-out residual overstates a frame's
    own error by t / (t - 1): 0.41 px for three frames), relative to the
    reference frame; patch cases add a local part of up to 0.2 px (y) and 0.3 px (x) across the frame."""
    t = case.shape[0]
    f = np.arange(t) - t // 2
    a = case.amp
    dy = np.round(np.linspace(-a, a + 1, t)) + case.frac * np.sin(1.3 * f)
    dx = np.round(np.linspace(a, 1 - a, t)) - 0.8 * case.frac * np.sin(0.9 * f + 0.4)
    rigid = np.stack([dy, dx], axis=1)
    rigid = rigid - rigid[ref_frame(case)]
    slope = np.stack([0.2 * np.sin(0.8 * f), -0.3 * f / max(t // 2, 1)], axis=1)
    return rigid, slope


def planted(case):
    """-> the fp32 movie (t, h, w) on the CPU."""
    t, h, w = case.shape
    rigid, slope = planted_drifts(case)
    if case.kind == "frame":
        return gr.planted_movie(t, h, w, rigid[:, 0], rigid[:, 1], noise=case.noise, seed=h + w + case.seed, band=case.tex)[0]
    return lr.planted_local_movie(t, h, w, rigid, slope, noise=case.noise, seed=h + w + case.seed, band=case.tex, waves=400)[0]


def raw_counts(case):
    """(raw u8 / i16 (t, h, w), gain (h, w) fp32 in 1 +- 0.1) of the planted movie, as tests/test_global_refine.py."""
    movie = planted(case)
    _, h, w = case.shape
    g = torch.Generator().manual_seed(5)
    gain = 1.0 + 0.1 * (2 * torch.rand(h, w, generator=g) - 1)
    if case.store == "u8":
        raw = ((20 * movie + 110) / gain).round().clamp(0, 255).to(torch.uint8)
    else:
        raw = ((300 * movie - 200) / gain).round().clamp(-32768, 32767).to(torch.int16)
    return raw, gain


def inputs(case):
    """What the route is called with -> dict(movie (fp32 / fp16 / raw), gain or None, field (2, t, 1, 1) fp32 or None)."""
    if case.store in RAW_KINDS:
        movie, gain = raw_counts(case)
    else:
        movie, gain = planted(case), None
        if case.store == "f16":
            movie = movie.half()
    field = None
    if case.kind == "patch":
        field = torch.from_numpy(np.rint(planted_drifts(case)[0]) * case.ps).float().T[:, :, None, None].contiguous()
    return dict(movie=movie, gain=gain, field=field)


# ------------------------------------------------------------------ one iteration of the restatement, its Jacobian


class _Patch:
    """One independent problem of the chain: whole frames, or one patch.  full (t, H, W // 2 + 1) the float64 spectra
    in numpy's layout, pruned (t, nkx, nky) the same on the kept bins, rel (t,) rel_S of each job, o (t, 2) the
    window offsets (zeros for whole frames)."""

    def __init__(self, kind, pa, pruned, rel, o, ref):
        self.kind, self.pa, self.pruned, self.rel, self.o, self.ref = kind, pa, pruned, rel, o, ref
        self.full = np.stack([xr.full_spectrum(s, pa) for s in pruned])
        self.H, self.W = int(pa[0]), int(pa[1])

    def iterate(self, s, n=1, full=None, dtype=np.float64, fault=None):
        """n iterations of the restatement from s (t, 2) -> (shifts, [r per iteration], [parabola offsets]).  `full`:
        other spectra in the same layout; `dtype`, `fault`: handed to the restatement."""
        full = self.full if full is None else full
        if self.kind == "frame":
            res = []
            out, _, offs = gr.refine_shifts(full, (self.H, self.W), self.ref, start=s, max_iterations=n,
                                            threshold=0.0, residuals=res, dtype=dtype, fault=fault)
            return out, res, offs
        out, _, offs, res = lr.refine_patches(full[:, None], self.H, s[:, None], self.o[:, None], self.ref, n, 0.0,
                                              dtype=dtype, fault=fault)
        return out[:, 0], [r[:, 0] for r in res], [o[:, 0] for o in offs]


def jacobians(patch, s, live, step):
    """Central differences of one iteration of the restatement at s (t, 2) over the inputs `live` (flat indices into
    (t, 2)) -> (|J| (2t, 2t), |R| (2t, 2t)), zero columns elsewhere."""
    n = s.size
    J, R = np.zeros((n, n)), np.zeros((n, n))
    for j in live:
        d = np.zeros(n)
        d[j] = step
        sp, rp, _ = patch.iterate(s + d.reshape(s.shape))
        sm, rm, _ = patch.iterate(s - d.reshape(s.shape))
        J[:, j] = np.abs((sp - sm).ravel()) / (2 * step)
        R[:, j] = np.abs((rp[0] - rm[0]).ravel()) / (2 * step)
    return J, R


def assert_patches_do_not_couple(case_name):
    """The restatement couples frames, not patches: moving the shifts of patch 0 leaves every other patch's next shifts
    bit-unchanged (and moves patch 0's)."""
    c = reference(case_name)
    full = np.stack([p.full for p in c["patches"]], axis=1)
    o = np.stack([p.o for p in c["patches"]], axis=1)
    s = c["start"].copy()
    assert s.shape[1] > 1
    base = lr.refine_patches(full, c["case"].p, s, o, c["ref"], 1, 0.0)[0]
    s[:, 0] += 1e-3
    moved = lr.refine_patches(full, c["case"].p, s, o, c["ref"], 1, 0.0)[0]
    assert np.array_equal(base[:, 1:], moved[:, 1:]) and not np.array_equal(base[:, 0], moved[:, 0])


# ------------------------------------------------------------------ the local error of one iteration


def kept_frequencies(pa):
    """Exact (fy (nky,), fx (nkx,)) of the kept bins in cycles / pixel, in the order of the pruned layout."""
    g = xr.geometry(pa)
    rows = xr.kept_rows(g)
    kk = np.where(rows < (g.H + 1) // 2, rows, rows - g.H).astype(np.float64)
    return kk / g.H, np.arange(g.nkx, dtype=np.float64) / g.W


def local_error(patch, s, under):
    """One iteration from s (t, 2) by the per-kernel float64 definitions, with the bounds of the module docstring.
    -> dict(new (t, 2), delta (t, 2), r (t, 2), delta_r (t, 2), off (t, 2), unique, inside, den_ok, E)."""
    S, pa, ref = patch.pruned, patch.pa, patch.ref
    t = S.shape[0]
    fy, fx = kept_frequencies(pa)
    d = s - patch.o
    d_err = (2 * U + (U if patch.kind == "patch" else 0.0)) * np.abs(d)
    Gu, REF, eG, eREF = ir._aligned(S, d, fy, fx, under, d_err)
    eG = eG + np.abs(S) * 2 * np.pi * 2 * U * under * (np.abs(fy)[None, :] + np.abs(fx)[:, None])
    nS = np.array([np.linalg.norm(x) for x in S])
    peaks, nbs, pb = np.zeros(t, dtype=np.int64), np.zeros((t, 3, 3)), np.zeros((t, 2))
    unique = inside = den_ok = True
    Es = []
    for f in range(t):
        cc = xr.correlation64(Gu[f], REF[f], pa)
        rel_cur = patch.rel[f] + np.linalg.norm(eG[f]) / np.linalg.norm(Gu[f])
        others = sum(patch.rel[g] * nS[g] for g in range(t) if g != f) / (t - 1)
        rel_ref = (others + np.linalg.norm(eREF[f])) / np.linalg.norm(REF[f])
        _, E = xr.map_bounds(pa, rel_cur, rel_ref, cc)
        Es.append(E)
        peaks[f] = int(np.argmax(cc))
        unique &= len(xr.admissible(cc, E)) == 1
        nb = xr.neighbourhood64(cc, peaks[f])
        inside &= not np.isnan(nb).any()
        nbs[f] = nb
        pb[f] = (xr.parabola_bound(nb[0, 1], nb[1, 1], nb[2, 1], E), xr.parabola_bound(nb[1, 0], nb[1, 1], nb[1, 2], E))
    den_ok = bool(np.isfinite(pb).all())
    r, e_r, off = ir.residuals64(peaks, nbs, patch.H, patch.W, under)
    damp = ir.damp32(t)
    delta_r = e_r + pb
    new, delta = ir._recentre(s, r, delta_r, ref, damp)
    delta = delta + U * np.abs(damp * r) + U * np.abs(damp * r[ref])
    delta[ref] = 0.0
    return dict(new=new, delta=delta, r=r, delta_r=delta_r, off=off, unique=bool(unique), inside=bool(inside),
                den_ok=den_ok, E=max(Es))


def chain_bound(patch, start, e0, under, iterations=ITER):
    """The recursion of the module docstring for one patch -> dict(field (t, 2) the composed definitions' shifts, bound
    (t, 2), hist (iterations,) max |r| of this patch, hbound (iterations,), r [..], off [..], normJ [..], agree [..],
    sum_delta, conditions)."""
    s, e = np.array(start, dtype=np.float64), np.array(e0, dtype=np.float64)
    out = dict(hist=[], hbound=[], r=[], off=[], normJ=[], agree=[], sum_delta=0.0, unique=True, inside=True, den_ok=True)
    for _ in range(iterations):
        le = local_error(patch, s, under)
        live = np.nonzero(e.ravel() > 0)[0]
        if len(live):
            (Ja, Ra), (Jb, Rb) = (jacobians(patch, s, live, h) for h in STEPS)
            J, R = np.maximum(Ja, Jb), np.maximum(Ra, Rb)
            for a, b, m in ((Ja, Jb, J), (Ra, Rb, R)):  # || |Ja| - |Jb| ||_inf against ||J||_inf, and the same for R
                out["agree"].append(float(np.abs(a - b).sum(axis=1).max() / max(m.sum(axis=1).max(), 1e-300)))
            out["normJ"].append(float(J.sum(axis=1).max()))
            e_next = (J @ e.ravel()).reshape(e.shape) + le["delta"]
            e_r = (R @ e.ravel()).reshape(e.shape) + le["delta_r"]
        else:
            out["normJ"].append(None)  # multiplies e = 0
            e_next, e_r = le["delta"], le["delta_r"]
        e_next[patch.ref] = 0.0
        out["hist"].append(float(np.abs(le["r"]).max()))
        out["hbound"].append(float(e_r.max()))
        out["r"].append(le["r"])
        out["off"].append(le["off"])
        out["sum_delta"] += float(le["delta"].max())
        for k in ("unique", "inside", "den_ok"):
            out[k] &= le[k]
        s, e = le["new"], e_next
    out["field"], out["bound"] = s, e
    return out


# ------------------------------------------------------------------ a case's spectra, start and reference


def _frame_spectra(case, stats):
    """-> (pa, pruned (t, nkx, nky), rel (t,)) of a whole-frame case; `stats` = (sub (t,), rstd) for raw counts."""
    t, h, w = case.shape
    pa = xr.args(h, w, case.ps, case.freq)
    if case.store in RAW_KINDS:
        raw, gain = raw_counts(case)
        sub, rstd = xr.raw_stats64(raw, gain) if stats is None else (np.asarray(stats[0], dtype=np.float32), float(stats[1]))
        v = condition_float64(raw.numpy(), gain.numpy(), sub)
        parts = xr.spectra_parts(v, pa, stats=(0.0, 1.0 / float(rstd)))
        mask = xr.tables64(pa)[0]
        rel = []
        for f in range(t):
            c = np.linalg.norm(conditioning_error(raw[f].numpy(), gain.numpy(), sub[f]) * mask) / np.linalg.norm(v[f] * mask)
            rel.append(xr.spectra_bounds(pa, 0.0, 1.0 / float(rstd), conditioning=float(c))["rel"])
        return pa, parts["S"], np.array(rel)
    x = inputs(case)["movie"].float()
    parts = xr.spectra_parts(x, pa)
    kinds = xr.line_costs(xr.geometry(pa))["kinds"]
    fused = None
    if kinds["rows"] == "native" and kinds["cols"] == "native":  # the fused-statistics route may run: the larger bound
        m0 = float(x[0, int(0.25 * h), int(0.25 * w):int(0.75 * w)].double().mean())
        fused = (abs(parts["mean"] - m0) / parts["std"], xr.mask_spectrum64(pa))
    b = xr.spectra_bounds(pa, parts["mean"], parts["std"], fused=fused)
    rel = np.array([b["rel"] + b["fix_l2"] / np.linalg.norm(s) for s in parts["S"]])
    return pa, parts["S"], rel


def _patch_spectra(case, s0):
    """-> (pa, pruned (t, npatch, nkx, nky), rel (t, npatch), offsets (t, npatch, 2)) of a patch case."""
    t, h, w = case.shape
    p = case.p
    pa = xr.args(p, p, case.ps, case.freq)
    cond = None
    if case.store in RAW_KINDS:  # the conditioned route: condition_movie, then the fp32 route
        raw, gain = raw_counts(case)
        mu = (raw.double().numpy() * gain.double().numpy()).mean(axis=(1, 2)).astype(np.float32)
        x = condition_float64(raw.numpy(), gain.numpy(), mu)
        cond = conditioning_error(raw.numpy(), gain.numpy(), mu) + U * np.abs(mu.astype(np.float64))[:, None, None]
    else:
        x = inputs(case)["movie"].float().double().numpy()
    mean, std = xr.box_stats64(x)
    _, _, origin = lr.patch_lattice(case.shape, p)
    o = lr.window_offsets(s0, case.shape, p)
    jobs = [(f, int(origin[q, 0] + o[f, q, 0]), int(origin[q, 1] + o[f, q, 1])) for f in range(t) for q in range(len(origin))]
    parts = xr.spectra_parts(x, pa, jobs, stats=(mean, std))
    mask = xr.tables64(pa)[0]
    rel = []
    for f, y0, x0 in jobs:
        c = 0.0
        if cond is not None:
            win = (f, slice(y0, y0 + p), slice(x0, x0 + p))
            c = float(np.linalg.norm(cond[win] * mask) / np.linalg.norm((x[win] - mean) * mask))
        rel.append(xr.spectra_bounds(pa, mean, std, conditioning=c)["rel"])
    n = len(origin)
    return pa, parts["S"].reshape((t, n) + parts["S"].shape[1:]), np.array(rel).reshape(t, n), o.astype(np.float64)


@functools.lru_cache(maxsize=None)
def _reference(name, stats):
    case = CASES[name]
    t, h, w = case.shape
    ref = ref_frame(case)
    inp = inputs(case)
    if case.kind == "frame":
        pa, S, rel = _frame_spectra(case, stats)
        patches = [_Patch("frame", pa, S, rel, np.zeros((t, 2)), ref)]
        full = patches[0].full
        start = gr.integer_shifts(full, (h, w), ref)[:, None]
        e0 = np.zeros_like(start)
        field = None
        if case.start == "caller":
            base, _, _ = patches[0].iterate(start[:, 0], 10)
            sign = (-1.0) ** np.arange(t)
            want = base + np.stack([0.4 * sign, -0.3 * sign], axis=1)
            field = torch.from_numpy((want * case.ps).astype(np.float32)).T[:, :, None, None].contiguous()
            start = (field.double()[:, :, 0, 0].T.numpy() / case.ps)[:, None]
            e0 = U * np.abs(start)  # the engine's fp32 quotient field / pixel spacing
        under = under_px(h, w)
    else:
        field = inp["field"]
        start = lr.start_px(field, case.ps, case.shape, case.p)
        e0 = SPLINE_ROUNDINGS * U * np.abs(start)
        pa, S, rel, o = _patch_spectra(case, start)
        patches = [_Patch("patch", pa, S[:, q], rel[:, q], o[:, q], ref) for q in range(S.shape[1])]
        under = under_px(case.p, case.p)
    npatch = len(patches)
    want = np.zeros((t, npatch, 2))
    res = []
    for q, p in enumerate(patches):
        want[:, q], _, _ = p.iterate(start[:, q], ITER)
        res.append(chain_bound(p, start[:, q], e0[:, q], under))
    composed = np.stack([r["field"] for r in res], axis=1)
    bound = np.stack([r["bound"] for r in res], axis=1)
    bound = bound + U * np.abs(want) * (bound > 0)  # the product with the pixel spacing on the way out
    per_iter = np.array([r["hist"] for r in res])       # (npatch, ITER)
    hist = per_iter.max(axis=0)
    hbound = np.array([r["hbound"] for r in res]).max(axis=0)  # |max a - max b| <= max |a - b|
    normJ = [max((r["normJ"][i] for r in res if r["normJ"][i] is not None), default=None) for i in range(ITER)]
    agree = max((a for r in res for a in r["agree"]), default=0.0)
    offs = max(float(np.abs(o).max()) for r in res for o in r["off"])
    rs = [x for r in res for x in r["r"]]
    return dict(case=case, ref=ref, inputs=inp, field=field, start=start, patches=patches, want=want, composed=composed,
                bound=bound, hist=hist, hbound=hbound, normJ=normJ, agree=agree, max_offset=offs,
                r_range=(min(float(x.min()) for x in rs), max(float(x.max()) for x in rs)),
                sum_delta=max(r["sum_delta"] for r in res), unique=all(r["unique"] for r in res),
                inside=all(r["inside"] for r in res), den_ok=all(r["den_ok"] for r in res), under=under, pa=pa)


def reference(name, stats=None):
    """Everything the tests need of the case `name`, computed once (and once more per `stats` = (sub, rstd) that a
    device hands over for raw counts, where they differ from xc_reference.raw_stats64's)."""
    if stats is not None:
        stats = (tuple(float(v) for v in stats[0]), float(stats[1]))
        raw, gain = raw_counts(CASES[name])
        sub, rstd = xr.raw_stats64(raw, gain)
        if stats == (tuple(float(v) for v in sub), float(rstd)):
            stats = None
    return _reference(name, stats)


def fitness(c):
    """The conditions on the inputs (module docstring); AssertionError names the one that fails."""
    name = c["case"].name
    assert c["max_offset"] <= MAX_OFFSET, f"{name}: a parabola offset of {c['max_offset']:.3f}"
    assert NEAR[0] < c["r_range"][0] and c["r_range"][1] < NEAR[1], f"{name}: residuals {c['r_range']} leave the near window"
    assert c["unique"], f"{name}: a second value within 2E of a map's maximum"
    assert c["inside"] and c["den_ok"], f"{name}: a neighbourhood leaves the map, or |den| <= 4E"
    assert c["agree"] <= J_AGREE, f"{name}: the two Jacobians differ by {c['agree']:.3f} in infinity norm"
    assert np.abs(c["composed"] - c["want"]).max() <= 1e-9, f"{name}: the composed definitions leave the restatement"
    assert not c["want"][c["ref"]].any() and not c["bound"][c["ref"]].any()
    assert math.isfinite(c["bound"].max()) and c["bound"].max() <= FINAL, f"{name}: final bound {c['bound'].max():.3e} px"
    assert np.abs(c["want"]).max() > 0.2, f"{name}: nothing to refine"


def check(c, shifts, hist, what):
    """A route's (or a stand-in's) (t, npatch, 2) px shifts and per-iteration max |r| against the case: every frame,
    patch and axis within its bound, the reference frame's row exactly 0, the history within its bound.
    -> (worst field ratio, [history ratio per iteration])."""
    shifts = np.asarray(shifts, dtype=np.float64).reshape(c["want"].shape)
    assert not shifts[c["ref"]].any(), f"{what}: the reference frame's row is not exactly 0"
    ratio = ir.assert_within(shifts, c["want"], c["bound"], f"{what} field")
    hist = np.asarray(hist, dtype=np.float64).reshape(-1)
    assert hist.shape == c["hist"].shape, (what, hist.shape)
    hr = [ir.assert_within(hist[k:k + 1], c["hist"][k:k + 1], c["hbound"][k:k + 1], f"{what} max |r| of iteration {k}")
          for k in range(len(hist))]
    return ratio, hr


def table_row(c, standin=None):
    nj = ", ".join("-" if v is None else f"{v:.3f}" for v in c["normJ"])
    s = "" if standin is None else f" | {standin:.3f}"
    return (f"| {c['case'].name} | {nj} | {c['sum_delta']:.2e} | {c['bound'].max():.2e} | "
            f"{max(c['hbound']):.2e}{s} |")
