"""float64 definitions, derived bounds and shared cases for the kernels of the iterative estimators
(csrc/local_motion.hip: mc_local_loss_sums, mc_local_ncc_grad; csrc/xc_refine.hip: mc_xc_aligned_refs,
mc_xc_refine_update; csrc/xc_refine_patches.hip: their _patches forms).  tests/test_iteration_reference_host.py checks
this file on the host (the definitions against the losses and estimators they serve, an fp32 stand-in in the kernels'
order of operations, deliberately wrong stand-ins that every comparison must reject);
tests/test_iteration_kernels_float64.py runs the same comparisons on the kernels' output.

TEST INFRASTRUCTURE ONLY: numpy on the CPU.  The inputs are the fp32 arrays exactly as a kernel receives them, taken
at their float64 value; fp32 constants a kernel receives or forms from integers (damp = (t - 1) / t) are taken at
their fp32 value.  Definitions (include/mcorr.h), bins kx-major (k = kx * nky + ky):

  loss_sums64       G_f = P_f exp(-2 pi i (fy sy_f + fx sx_f)), S = sum_f G_f and, per (patch, frame), the six sums
                    over the bins  h fy Im(conj(S) G_f), h fx Im(conj(S) G_f), h |t G_f - S|^2, h Re(G_f conj(S - G_f)),
                    h |S - G_f|^2, h |G_f|^2  (h = hx[kx], 1 without hx).
  ncc_grad_sums64   R_f = (S - G_f) / (t - 1), C_f = a_f conj(G_f) + 2 b_f conj(R_f), C = sum_f C_f,
                    V_f = a_f conj(R_f) + (C - C_f) / (t - 1), the sums h fy Im(V_f G_f) and h fx Im(V_f G_f).
  aligned_refs64    G_f = S_f exp(+2 pi i (fy sy_f + fx sx_f)), A = sum_f G_f, REF_f = (A - G_f) / (t - 1) (0 for
                    t = 1), G'_f = G_f exp(-2 pi i under (fy + fx)); the patch form carries s - o per (frame, patch) and
                    writes the patches [q0, q0 + nq) only, [t][nq][bins].
  refine_update64   r = wrap((peak - under) mod n) + parabola offset (guards: both outer samples not NaN and unequal),
                    s_f += damp r_f, s -= s_ref with row ref exactly 0, max_r = max |r|; the patch form per patch of
                    the range, everything outside the range untouched.

BOUNDS, u = 2^-24.  Every bound is a sum of named first-order terms, absolute, per output element, formed from the
magnitudes of the terms that are added (sum |term|), never from the size of the result: the sums cancel to zero for an
aligned stack.  No bound is fitted to a kernel's output, no element is left out of a comparison.

 Loss kernels (local_motion.hip is compiled with the default contraction, so every count below covers the expression
 with and without fused multiply-adds: a fused form has fewer roundings, never more).  Per bin and frame, m = |P_f|:
  angle     x = -2 (fy sy + fx sx) in half revolutions: fl(fy sy) and fl(fx sx) round at u |fy sy|, u |fx sx|, the sum at
            u |fy sy + fx sx| (fused: one product and the sum); the doubling is exact.  At most 2 u M, M = |fy sy| +
            |fx sx|, of the bracket, 4 u M of x, 4 pi u M radians.  The dominant term at large shifts.
  sincospi  OpenCL requires sinpi / cospi within 4 ulp and OCML is built to that profile; no accuracy table of OCML
            was found in the ROCm installation, so 4 ulp is an ASSUMPTION of this file: 4 * 2^-23 absolute per
            component (ulp of a value <= 1), sqrt2 times that in modulus.  sincospi reduces its argument exactly
            (x - 2 rint(x / 2) is a float), which is the "exact range reduction for large shifts" of the kernel's
            comment: the large-shift cases test it, no term stands for it.
  product   g = p (c + i s): two roundings per component, sqrt2 gamma_2 |p| = 2 sqrt2 u m in modulus.
            e_f = m (4 pi u M + sqrt2 SINCOSPI + 2 sqrt2 u)  bounds |g_f - G_f| for either evaluation of g.
  S         t - 1 fp32 additions per component over partial sums bounded by MS = sum_f m_f (Minkowski for the
            modulus):  eS = sum_f e_f + (t - 1) u MS.
  terms     with |S| <= MS, |S - G| <= MS, |t G - S| <= MD = t m + MS, each a perturbation (first line) and the
            roundings of its own arithmetic (second):
              Im(conj(S) G)        eS m + MS e;                     2 u MS m, and 2 u more for h f * (.)
              t G - S              eD = t e + eS + u (t m + MD)     (the product by t and the subtraction)
              h |t G - S|^2        2 MD eD;                         3 u MD^2 (two squares and a sum: 2u; h: u)
              S - G                eR = eS + e + u MS
              h Re(G conj(S - G))  e MS + m eR;                     3 u m MS
              h |S - G|^2          2 MS eR;                         3 u MS^2
              h |G|^2              2 m e;                           3 u m^2
  sums      a lane adds its 16 bins of the tile in sequence and the wave reduction adds six more levels: 22 u times
            sum |term| over the tile.  The Python layer adds the tiles in float64; the comparison is per tile (the
            kernel's partial against the float64 sum over that tile's bins), which is the stronger statement and
            shows a wrong tile stride where a total might not.
  ncc       inv = fl(1 / (t - 1)) within 2 u (one ulp: the division is not assumed correctly rounded), bf = 2 b inv
            within 3 u;  alpha = |a|, beta = 2 |b| / (t - 1), MCf = alpha m + beta MS, MC = sum_f MCf:
              C_f      eCf = alpha e + beta eR + 3 u beta MS + 2 u MCf
              C        eC = sum_f eCf + t u MC                       (t additions)
              R        eRn = eR / (t - 1) + 3 u MS / (t - 1)
              W = (C - C_f) / (t - 1)   eW = (eC + eCf + u MC + 3 u MC) / (t - 1)
              V        eV = alpha eRn + eW + 2 u MV,  MV = alpha MS / (t - 1) + MC / (t - 1)
              h f Im(V G)   h |f| (eV m + MV e + 4 u MV m), then the 22 u of the sums.

 mc_xc_aligned_refs (fp contract off: the roundings are exactly the written ones), per bin, in modulus:
  cis       fl(fy sy) in revolutions: 2 pi u |fy sy| radians; v_fract is exact for a non-negative argument and
            rounds 1 + x once for a negative one: 2 pi u (a term the first derivation lacked); the transcendental unit:
            1e-6 absolute per component (mc_common.h), sqrt2 1e-6 in modulus, as the Fourier pin takes it.
            eps(z) = 2 pi u |z| + 2 pi u + sqrt2 1e-6.
  ramp      the product of the two cis with written-out fmas: 2 sqrt2 u;   s times the ramp: 2 sqrt2 u more:
            e_f = m (eps(fy sy) + eps(fx sx) + 4 sqrt2 u),  m = |S_f|.
  A         t - 1 additions: eA = sum_f e_f + (t - 1) u MA, MA = sum_f m_f.
  REF       the subtraction u MA, the product with inv 3 u MA / (t - 1) (inv within 2 u, the product u):
            eREF = (eA + e + u MA + 3 u MA) / (t - 1); exactly 0 for t = 1.
  under     E = cis(-fl(fy under)) cis(-fl(fx under)): eps(fy under) + eps(fx under) + 2 sqrt2 u, then g E: 2 sqrt2 u:
            eG = e + m (eps(fy under) + eps(fx under) + 4 sqrt2 u).
  s - o     the patch form rounds d = s - o once: u |d| in pixels, 2 pi u |f d| more in each eps.

 mc_xc_refine_update (fp contract off).  The integer residual is exact.  The parabola offset is the chain of
 xc_reference.accumulate64: n = v0 - v2 (u |off|), a = v0 - 2 v1 and den = a + v2 (amp u |off|, amp = (|a| + |den|) /
 |den|, the denominator's cancellation), the quotient (u |off|), r = i + off (u |r|):
              e_r = (2 + amp) u |off| + u |r|
 then damp r (u |damp r|), s + damp r (u |s'|), and the re-centring s'_f - s'_ref (u of the difference):
              e_s = damp e_r + u |damp r| + u |s'|,   bound = e_s(f) + e_s(ref) + u |s'_f - s'_ref|,
 row ref exactly 0, max_r within max e_r.  First order needs a denominator that is known: with E = u (|v0| + 2 |v1| +
 |v2|) (den is computed to within 2 E) every axis a case evaluates has |den| > 4 E -- a condition on the inputs,
 asserted on the host for every case; no axis is left out.
"""

from __future__ import annotations

import numpy as np

from kernel_harness import rng as _rng

F32 = np.float32
U = 2.0 ** -24
SQ2 = np.sqrt(2.0)
SINCOSPI = 4 * 2.0 ** -23   # 4 ulp of a value <= 1 (assumption, module docstring)
TRIG_UNIT = 1e-6            # mc_common.h: v_sin_f32 / v_cos_f32, absolute per component
LM_TILE = 1024
XR_WG = 256
SENTINEL = -7.5e8           # what the GPU tests pre-fill outputs with


def ntiles(nkx, nky):
    return (nkx * nky + LM_TILE - 1) // LM_TILE


def cplx(a):
    """(.., 2) fp32 pairs, or a complex array -> complex128."""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return a.astype(np.complex128)
    a = a.astype(np.float64)
    return a[..., 0] + 1j * a[..., 1]


def pairs(z):
    """complex -> (.., 2) fp32 pairs."""
    z = np.asarray(z)
    return np.stack([z.real, z.imag], axis=-1).astype(F32)


# ------------------------------------------------------------------ loss kernels: definitions and bounds


def _tiles(a, nt):
    """(npatch, t, nbins, c) per-bin terms -> (npatch, ntiles, t, c) sums over each tile's bins."""
    npatch, t, nbins, c = a.shape
    pad = np.zeros((npatch, t, nt * LM_TILE - nbins, c))
    a = np.concatenate([a, pad], axis=2).reshape(npatch, t, nt, LM_TILE, c).sum(axis=3)
    return np.ascontiguousarray(a.transpose(0, 2, 1, 3))


class _Shifted:
    """G (npatch, t, nkx, nky) complex128 and the magnitudes the bounds need."""

    def __init__(self, P, shifts, fy, fx, hx):
        P = cplx(P)
        npatch, t, nkx, nky = P.shape
        s = np.asarray(shifts, dtype=np.float64).reshape(npatch, t, 2)
        fy, fx = np.asarray(fy, dtype=np.float64), np.asarray(fx, dtype=np.float64)
        assert fy.shape == (nky,) and fx.shape == (nkx,)
        ay = fy[None, None, None, :] * s[:, :, 0, None, None]
        ax = fx[None, None, :, None] * s[:, :, 1, None, None]
        self.t, self.shape = t, P.shape
        self.G = P * np.exp(-2j * np.pi * (ay + ax))
        self.m = np.abs(P)
        self.e = self.m * (4 * np.pi * U * (np.abs(ay) + np.abs(ax)) + SQ2 * SINCOSPI + 2 * SQ2 * U)
        self.S = self.G.sum(axis=1, keepdims=True)
        self.MS = self.m.sum(axis=1, keepdims=True)
        self.eS = self.e.sum(axis=1, keepdims=True) + (t - 1) * U * self.MS
        self.eR = self.eS + self.e + U * self.MS
        h = np.ones(nkx) if hx is None else np.asarray(hx, dtype=np.float64)
        assert h.shape == (nkx,)
        self.h = np.broadcast_to(h[None, None, :, None], P.shape)
        self.fy = np.broadcast_to(fy[None, None, None, :], P.shape)
        self.fx = np.broadcast_to(fx[None, None, :, None], P.shape)

    def tiles(self, terms, errs, mags):
        npatch, t, nkx, nky = self.shape
        nt = ntiles(nkx, nky)
        flat = lambda xs: np.stack([np.broadcast_to(x, self.shape).reshape(npatch, t, nkx * nky) for x in xs], axis=-1)
        return _tiles(flat(terms), nt), _tiles(flat(errs), nt) + 22 * U * _tiles(flat(mags), nt)


def loss_tiles64(P, shifts, fy, fx, hx):
    """-> (partial (npatch, ntiles, t, 6) float64, bound of the same shape): mc_local_loss_sums per tile."""
    q = _Shifted(P, shifts, fy, fx, hx)
    t, G, S, m, e, MS, eS, eR, h = q.t, q.G, q.S, q.m, q.e, q.MS, q.eS, q.eR, q.h
    im = (np.conj(S) * G).imag
    D, R = t * G - S, S - G
    MD = t * m + MS
    eD = t * e + eS + U * (t * m + MD)
    e_im = eS * m + MS * e + 4 * U * MS * m
    afy, afx = np.abs(q.fy), np.abs(q.fx)
    terms = [h * q.fy * im, h * q.fx * im, h * np.abs(D) ** 2, h * (G * np.conj(R)).real, h * np.abs(R) ** 2,
             h * np.abs(G) ** 2]
    errs = [h * afy * e_im, h * afx * e_im, h * (2 * MD * eD + 3 * U * MD ** 2),
            h * (e * MS + m * eR + 3 * U * m * MS), h * (2 * MS * eR + 3 * U * MS ** 2), h * (2 * m * e + 3 * U * m ** 2)]
    mags = [h * afy * MS * m, h * afx * MS * m, h * MD ** 2, h * m * MS, h * MS ** 2, h * m ** 2]
    return q.tiles(terms, errs, mags)


def loss_sums64(P, shifts, fy, fx, hx):
    """(npatch, t, 6) float64: the six sums of mc_local_loss_sums over all bins."""
    return loss_tiles64(P, shifts, fy, fx, hx)[0].sum(axis=1)


def ncc_grad_tiles64(P, shifts, fy, fx, hx, ab):
    """-> (partial (npatch, ntiles, t, 2), bound): mc_local_ncc_grad per tile."""
    q = _Shifted(P, shifts, fy, fx, hx)
    t, G, S, m, e, MS, eS, eR, h = q.t, q.G, q.S, q.m, q.e, q.MS, q.eS, q.eR, q.h
    ab = np.asarray(ab, dtype=np.float64).reshape(q.shape[0], t, 2)
    a, b = ab[:, :, 0, None, None], ab[:, :, 1, None, None]
    inv = 1.0 / (t - 1)
    R = (S - G) * inv
    Cf = a * np.conj(G) + 2 * b * np.conj(R)
    C = Cf.sum(axis=1, keepdims=True)
    V = a * np.conj(R) + (C - Cf) * inv
    im = (V * G).imag
    al, be = np.abs(a), 2 * np.abs(b) * inv
    MCf = al * m + be * MS
    MC = MCf.sum(axis=1, keepdims=True)
    eCf = al * e + be * eR + 3 * U * be * MS + 2 * U * MCf
    eC = eCf.sum(axis=1, keepdims=True) + t * U * MC
    eRn = eR * inv + 3 * U * MS * inv
    eW = (eC + eCf + 4 * U * MC) * inv
    MV = (al * MS + MC) * inv
    eV = al * eRn + eW + 2 * U * MV
    e_im = eV * m + MV * e + 4 * U * MV * m
    afy, afx = np.abs(q.fy), np.abs(q.fx)
    return q.tiles([h * q.fy * im, h * q.fx * im], [h * afy * e_im, h * afx * e_im], [h * afy * MV * m, h * afx * MV * m])


def ncc_grad_sums64(P, shifts, fy, fx, hx, ab):
    """(npatch, t, 2) float64: the two sums of mc_local_ncc_grad over all bins."""
    return ncc_grad_tiles64(P, shifts, fy, fx, hx, ab)[0].sum(axis=1)


# ------------------------------------------------------------------ aligned refs: definitions and bounds


def _eps(z):
    return 2 * np.pi * U * np.abs(z) + 2 * np.pi * U + SQ2 * TRIG_UNIT


def _aligned(S, d, fy, fx, under, d_err):
    """S (t, .., nkx, nky) complex128; d (t, .., 2) the shift the ramp carries, broadcast over the bins; d_err the
    rounding of d itself in pixels.  -> (G', REF, bound G', bound REF)."""
    t = S.shape[0]
    fy, fx = np.asarray(fy, dtype=np.float64), np.asarray(fx, dtype=np.float64)
    fyb, fxb = fy[None, :], fx[:, None]
    dy, dx = d[..., 0, None, None], d[..., 1, None, None]
    ey, ex = d_err[..., 0, None, None], d_err[..., 1, None, None]
    G = S * np.exp(2j * np.pi * (fyb * dy + fxb * dx))
    m = np.abs(S)
    e = m * (_eps(fyb * dy) + _eps(fxb * dx) + 2 * np.pi * (np.abs(fyb) * ey + np.abs(fxb) * ex) + 4 * SQ2 * U)
    A, MA = G.sum(axis=0, keepdims=True), m.sum(axis=0, keepdims=True)
    eA = e.sum(axis=0, keepdims=True) + (t - 1) * U * MA
    if t > 1:
        REF = (A - G) / (t - 1)
        eREF = (eA + e + 4 * U * MA) / (t - 1)
    else:
        REF, eREF = np.zeros_like(G), np.zeros_like(m)
    Gu = G * np.exp(-2j * np.pi * under * (fyb + fxb))
    eG = e + m * (_eps(fyb * under) + _eps(fxb * under) + 4 * SQ2 * U)
    return Gu, REF, eG, eREF


def aligned_refs64(S, shifts, fy, fx, under, bounds=False):
    """S (t, nkx, nky); shifts (t, 2) -> (G', REF) complex128 (t, nkx, nky) [, their bounds in modulus]."""
    S = cplx(S)
    d = np.asarray(shifts, dtype=np.float64).reshape(S.shape[0], 2)
    out = _aligned(S, d, fy, fx, under, np.zeros_like(d))
    return out if bounds else out[:2]


def aligned_refs_patches64(S, shifts, offsets, fy, fx, under, q0, nq, bounds=False):
    """S (t, npatch, nkx, nky); shifts, offsets (t, npatch, 2) -> (G', REF) (t, nq, nkx, nky) of patches [q0, q0 + nq)."""
    S = cplx(S)[:, q0:q0 + nq]
    t = S.shape[0]
    d = (np.asarray(shifts, dtype=np.float64) - np.asarray(offsets, dtype=np.float64)).reshape(t, -1, 2)[:, q0:q0 + nq]
    out = _aligned(S, d, fy, fx, under, U * np.abs(d))
    return out if bounds else out[:2]


def assert_complex_within(got, ref, bound, what):
    """|got - ref| <= bound in modulus at every element (NaN and untouched sentinels fail) -> worst ratio."""
    d = np.abs(cplx(got) - ref)
    bad = ~(d <= bound)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} bins beyond the bound, first at {i}: got {cplx(got)[i]!r} "
                             f"ref {ref[i]!r} bound {bound[i]!r}")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nan_to_num(d / bound, nan=0.0, posinf=0.0).max(initial=0.0))


def assert_within(got, ref, bound, what):
    """|got - ref| <= bound at every element (NaN fails) -> worst ratio."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), got.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d = np.abs(got - ref)
    bad = ~(d <= bound)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} values beyond the bound, first at {i}: got {got[i]!r} "
                             f"ref {ref[i]!r} bound {bound[i]!r}")
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nan_to_num(d / bound, nan=0.0, posinf=0.0).max(initial=0.0))


def check_aligned(G, REF, ref4, what):
    """The kernel's (or a stand-in's) G', REF (.., 2) fp32 against aligned_refs*64(.., bounds=True).  -> (ratio G',
    ratio REF); REF exactly 0 where its bound is 0 (t = 1)."""
    Gu, R, eG, eR = ref4
    rg = assert_complex_within(G, Gu, eG, f"{what} G'")
    if Gu.shape[0] == 1:
        assert not np.asarray(REF).any(), f"{what}: REF is not exactly 0 for one frame"
        return rg, 0.0
    return rg, assert_complex_within(REF, R, eR, f"{what} REF")


# ------------------------------------------------------------------ update kernels: definitions and bounds


def damp32(t):
    return float(F32(t - 1) / F32(t))


def parabola_den_condition(nb):
    """For (n, 3, 3) neighbourhoods: (evaluated (n, 2) bool, ok (n, 2) bool) -- which axes the guards let through and
    whether |den| > 4 E there, E = u (|v0| + 2 |v1| + |v2|)."""
    q = np.asarray(nb, dtype=np.float64).reshape(-1, 3, 3)
    ev, ok = np.zeros((len(q), 2), dtype=bool), np.ones((len(q), 2), dtype=bool)
    for c, (v0, v1, v2) in enumerate(((q[:, 0, 1], q[:, 1, 1], q[:, 2, 1]), (q[:, 1, 0], q[:, 1, 1], q[:, 1, 2]))):
        with np.errstate(invalid="ignore"):
            ev[:, c] = ~np.isnan(v0) & ~np.isnan(v2) & (v2 != v0)
            E = U * (np.abs(v0) + 2 * np.abs(v1) + np.abs(v2))
            ok[:, c] = ~ev[:, c] | (np.abs(v0 - 2 * v1 + v2) > 4 * E)
    return ev, ok


def residuals64(peaks, nb, H, W, under):
    """-> (r (n, 2) float64 (y, x), e_r (n, 2), off (n, 2)) of n pairs."""
    pk = np.asarray(peaks, dtype=np.int64).reshape(-1)
    q = np.asarray(nb, dtype=np.float64).reshape(-1, 3, 3)
    r, e_r, off = np.zeros((len(pk), 2)), np.zeros((len(pk), 2)), np.zeros((len(pk), 2))
    ev, _ = parabola_den_condition(q)
    for c, (n, (v0, v1, v2)) in enumerate(((H, (q[:, 0, 1], q[:, 1, 1], q[:, 2, 1])), (W, (q[:, 1, 0], q[:, 1, 1], q[:, 1, 2])))):
        i = ((pk // W if c == 0 else pk % W) - under) % n
        i = np.where(i <= n // 2, i, i - n).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            a = v0 - 2 * v1
            den = a + v2
            o = np.where(ev[:, c], 0.5 * (v0 - v2) / den, 0.0)
            amp = np.where(ev[:, c], (np.abs(a) + np.abs(den)) / np.abs(den), 0.0)
        off[:, c], r[:, c] = o, i + o
        e_r[:, c] = (2 + amp) * U * np.abs(o) + U * np.abs(r[:, c]) * ev[:, c]
    return r, e_r, off


def _recentre(s, r, e_r, ref, damp):
    """s, r, e_r (t, 2) -> (new s, bound), row ref exactly 0."""
    s1 = s + damp * r
    e_s = damp * e_r + U * np.abs(damp * r) + U * np.abs(s1)
    new = s1 - s1[ref]
    bound = e_s + e_s[ref] + U * np.abs(new)
    new[ref], bound[ref] = 0.0, 0.0
    return new, bound


def refine_update64(peaks, nb, shifts, ref, H, W, under, damp=None, bounds=False):
    """-> (shifts (t, 2) float64, max_r) [, bound of the shifts (t, 2), bound of max_r, r (t, 2), offsets (t, 2)]."""
    s = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    t = len(s)
    r, e_r, off = residuals64(peaks, nb, H, W, under)
    new, bound = _recentre(s, r, e_r, ref, damp32(t) if damp is None else damp)
    out = (new, float(np.abs(r).max()))
    return out + (bound, float(e_r.max()), r, off) if bounds else out


def refine_update_patches64(peaks, nb, shifts, ref, q0, nq, H, W, under, max_r, bounds=False):
    """peaks (t * nq,), nb (t * nq, 3, 3) in pair order f * nq + (q - q0); shifts (t, npatch, 2) and max_r (npatch,) as
    they are before the call -> (shifts, max_r) after it, float64, entries outside the range as given
    [, bound of the shifts, bound of max_r: zero outside the range]."""
    s = np.asarray(shifts).astype(np.float64)
    t, npatch, _ = s.shape
    mr = np.asarray(max_r).astype(np.float64).copy()
    r, e_r, _ = residuals64(peaks, nb, H, W, under)
    r, e_r = r.reshape(t, nq, 2), e_r.reshape(t, nq, 2)
    bs, bm = np.zeros_like(s), np.zeros(npatch)
    for qc in range(nq):
        q = q0 + qc
        s[:, q], bs[:, q] = _recentre(s[:, q], r[:, qc], e_r[:, qc], ref, damp32(t))
        mr[q], bm[q] = np.abs(r[:, qc]).max(), e_r[:, qc].max()
    return (s, mr, bs, bm) if bounds else (s, mr)


def check_update(shifts, max_r, ref4, ref, what):
    """Kernel (or stand-in) output against refine_update64(.., bounds=True)[:4] -> (ratio shifts, ratio max_r)."""
    want, wmax, bound, bmax = ref4[:4]
    shifts = np.asarray(shifts).reshape(want.shape)
    assert not shifts[ref].any(), f"{what}: row ref is not exactly 0"
    return (assert_within(shifts, want, bound, f"{what} shifts"),
            assert_within(np.asarray(max_r, dtype=np.float64).reshape(-1)[:1], [wmax], [bmax], f"{what} max_r"))


def check_update_patches(shifts, max_r, before_s, before_m, ref4, ref, q0, nq, what):
    """Patch form: the range within its bounds, row ref exactly 0 there, everything outside the range bit-equal to
    what was there before."""
    want, wmax, bs, bm = ref4
    shifts, max_r = np.asarray(shifts), np.asarray(max_r)
    out = np.ones(shifts.shape[1], dtype=bool)
    out[q0:q0 + nq] = False
    assert np.array_equal(shifts[:, out].view(np.uint32), np.asarray(before_s)[:, out].view(np.uint32)), \
        f"{what}: shifts outside the range changed"
    assert np.array_equal(max_r[out].view(np.uint32), np.asarray(before_m)[out].view(np.uint32)), \
        f"{what}: max_r outside the range changed"
    assert not shifts[ref, q0:q0 + nq].any(), f"{what}: row ref is not exactly 0"
    return (assert_within(shifts[:, ~out], want[:, ~out], bs[:, ~out], f"{what} shifts"),
            assert_within(max_r[~out], wmax[~out], bm[~out], f"{what} max_r"))


# ------------------------------------------------------------------ shared cases


def freqs(nkx, nky):
    """fp32 (fy (nky,), fx (nkx,)): the kept rows 0 .. kyp - 1 then -kyn .. -1 of a patch of height 2 nky + 3 (so fy
    holds negative rows whenever nky > 1) and the columns 0 .. nkx - 1 of a patch of width 2 nkx."""
    kyp = (nky + 1) // 2
    kk = np.concatenate([np.arange(kyp), np.arange(kyp - nky, 0)]).astype(F32)
    return kk * F32(1.0 / (2 * nky + 3)), np.arange(nkx, dtype=F32) * F32(1.0 / (2 * nkx))


# (npatch, t, nkx, nky): see the table of tests/test_iteration_kernels_float64.py
LOSS_CASES = [(1, 2, 1, 1), (2, 5, 5, 9), (3, 3, 16, 64), (2, 4, 25, 41), (2, 7, 33, 65), (1, 3, 1100, 1), (1, 3, 1, 1100),
              (1, 130, 3, 7), (1, 512, 7, 10)]
HX_FORMS = ("none", "hermitian", "arbitrary")
SHIFT_FORMS = ("zero", "half", "random", "large", "aligned")
LARGE_SHIFT = (-200.25, 180.5)


def make_hx(form, nkx, seed=0):
    if form == "none":
        return None
    if form == "hermitian":
        h = np.full(nkx, 2.0, dtype=F32)
        h[0] = h[-1] = 1.0
        return h
    return (0.5 + 2.5 * _rng(11, nkx, seed).random(nkx)).astype(F32)


def loss_case(case, shift_form, seed=0):
    """-> dict(P (npatch, t, nkx, nky, 2) fp32, shifts (npatch, t, 2) fp32, fy, fx, ab (npatch, t, 2) fp32): every
    patch and frame with its own spectrum and shift."""
    npatch, t, nkx, nky = case
    r = _rng(3, npatch, t, nkx, nky, SHIFT_FORMS.index(shift_form), seed)
    fy, fx = freqs(nkx, nky)
    P = r.normal(0, 1, (npatch, t, nkx, nky, 2)).astype(F32)
    if shift_form == "zero":
        s = np.zeros((npatch, t, 2))
    elif shift_form == "half":
        s = r.integers(-5, 6, (npatch, t, 2)) + 0.5
    else:
        s = r.uniform(-3, 3, (npatch, t, 2))
        if shift_form == "large":
            s[:, 0] = 0.0
            s += np.array(LARGE_SHIFT)
    s = s.astype(F32)
    if shift_form == "aligned":  # P_f = P_0 ramp(+s_f) in float64, rounded: every G_f is P_0 up to that rounding
        s[:, 0] = 0.0
        ang = fy.astype(np.float64)[None, None, None, :] * s[:, :, 0, None, None].astype(np.float64) \
            + fx.astype(np.float64)[None, None, :, None] * s[:, :, 1, None, None].astype(np.float64)
        P = pairs(cplx(P[:, :1]) * np.exp(2j * np.pi * ang))
    return dict(P=np.ascontiguousarray(P), shifts=s, fy=fy, fx=fx, ab=r.normal(0, 1, (npatch, t, 2)).astype(F32))


# (t, nkx, nky, under)
ALIGNED_CASES = [(1, 1, 1, 0), (2, 1, 1, 0), (6, 5, 9, 16), (3, 4, 64, 16), (5, 1, 257, 8), (4, 300, 1, 3), (67, 3, 7, 16),
                 (512, 2, 3, 16)]
PATCH_RANGES = [(0, 5), (2, 2), (4, 1)]
NPATCH = 5


def aligned_shifts(t, r):
    """(t, 2) fp32: both signs, fractions, whole pixels (fy sy is then a whole revolution at some bins) and the large
    shift, in turn."""
    s = r.uniform(-6, 6, (t, 2))
    s[1::4] = np.rint(s[1::4] / 2) * 8       # whole pixels, both signs: multiples of 8 up to 24
    s[2::4] = np.array(LARGE_SHIFT)
    return s.astype(F32)


def aligned_case(case, seed=0):
    t, nkx, nky, under = case
    r = _rng(5, t, nkx, nky, under, seed)
    fy, fx = freqs(nkx, nky)
    if nky > 1:  # a power-of-two height: the shifts of 8, 16, 24 px are whole revolutions at the rows k = height / 8 j
        kyp = (nky + 1) // 2
        height = 1 << int(np.ceil(np.log2(2 * nky + 3)))
        fy = np.concatenate([np.arange(kyp), np.arange(kyp - nky, 0)]).astype(F32) * F32(1.0 / height)
    return dict(S=r.normal(0, 1, (t, nkx, nky, 2)).astype(F32), shifts=aligned_shifts(t, r), fy=fy, fx=fx, under=under)


def aligned_patch_case(case, seed=0):
    """S (t, NPATCH, nkx, nky, 2), shifts and whole-pixel offsets (t, NPATCH, 2): offsets non-zero, and in patches 1
    and 4 within a fraction of the shift, so that s - o cancels."""
    t, nkx, nky, under = case
    c = aligned_case(case, seed)
    r = _rng(6, t, nkx, nky, under, seed)
    S = r.normal(0, 1, (t, NPATCH, nkx, nky, 2)).astype(F32)
    sh = np.stack([aligned_shifts(t, r) for _ in range(NPATCH)], axis=1)
    of = r.integers(-40, 41, (t, NPATCH, 2)).astype(np.float64)
    of[of == 0] = 7
    for q in (1, 4):
        frac = r.uniform(-0.5, 0.5, (t, 2))
        sh[:, q] = (of[:, q] + frac * (0.01 if q == 4 else 1.0)).astype(F32)
    return dict(S=S, shifts=np.ascontiguousarray(sh), offsets=of.astype(F32), fy=c["fy"], fx=c["fx"], under=under)


UPDATE_T = (2, 6, 64, 65, 130, 512)
UPDATE_SHAPES = (((96, 120), 16), ((9, 11), 3))  # ((H, W), under)


def update_refs(t):
    return (0, t // 2, t - 1)


def update_case(t, ref_variant, shape, under, seed=0):
    """One frame set of the update kernels -> dict(peaks (t,) int32, nb (t, 3, 3) fp32, shifts (t, 2) fp32, ref, big).
    ref = update_refs(t)[ref_variant]; the largest residual (a peak at exactly n / 2 on both axes with offsets
    of +0.44) lies in the last frame, in frame 0, in `ref` for variant 0, 1, 2.  The other frames take, in turn: the
    peak (under, under); positions below `under` (wrap below zero); n / 2 + 1 on both axes (offsets >= 0 there, so
    |r| stays below the big one); a NaN neighbour on the y axis only / the x axis only; v0 == v2; v0 == v1 == v2;
    ordinary peaks within 3 px."""
    H, W = shape
    ref = update_refs(t)[ref_variant]
    big = (t - 1, 0, ref)[ref_variant]
    r = _rng(7, t, ref_variant, H, W, seed)
    iy = under + r.integers(-3, 4, t)
    ix = under + r.integers(-3, 4, t)
    nb = np.empty((t, 3, 3))
    nb[:, 1, 1] = 1.0 + r.random(t)
    for i, j in ((0, 1), (2, 1), (1, 0), (1, 2), (0, 0), (0, 2), (2, 0), (2, 2)):
        nb[:, i, j] = nb[:, 1, 1] - r.uniform(0.1, 0.6, t)
    kinds = ["centre", "below", "half+1", "nan-y", "nan-x", "v0==v2", "flat", "plain"]
    kind = [kinds[f % len(kinds)] for f in range(t)]
    kind[big] = "big"
    for f, k in enumerate(kind):
        if k == "centre":
            iy[f], ix[f] = under, under
        elif k == "below":
            iy[f], ix[f] = under - 2, under - 1
        elif k == "half+1":
            iy[f], ix[f] = (H // 2 + 1 + under) % H, (W // 2 + 1 + under) % W
            nb[f, 0, 1], nb[f, 1, 0] = min(nb[f, 0, 1], nb[f, 2, 1]) - 0.05, min(nb[f, 1, 0], nb[f, 1, 2]) - 0.05
        elif k == "nan-y":
            nb[f, 0, :] = np.nan
        elif k == "nan-x":
            nb[f, :, 2] = np.nan
        elif k == "v0==v2":
            nb[f, 2, 1], nb[f, 1, 2] = nb[f, 0, 1], nb[f, 1, 0]
        elif k == "flat":
            nb[f] = nb[f, 1, 1]
        elif k == "big":
            iy[f], ix[f] = (H // 2 + under) % H, (W // 2 + under) % W
            nb[f, 1, 1] = 1.0
            nb[f, 0, 1] = nb[f, 1, 0] = 0.15
            nb[f, 2, 1] = nb[f, 1, 2] = 0.95
    peaks = (np.mod(iy, H) * W + np.mod(ix, W)).astype(np.int32)
    return dict(peaks=peaks, nb=nb.astype(F32), shifts=r.uniform(-8, 8, (t, 2)).astype(F32), ref=ref, big=big, kinds=kind)


def update_patch_case(t, ref_variant, shape, under, q0, nq, seed=0):
    """NPATCH independent frame sets; peaks / nb of the range in pair order; shifts (t, NPATCH, 2); max_r (NPATCH,)
    pre-filled."""
    cs = [update_case(t, ref_variant, shape, under, seed=100 + q) for q in range(NPATCH)]
    peaks = np.stack([cs[q]["peaks"] for q in range(q0, q0 + nq)], axis=1).reshape(-1)
    nb = np.stack([cs[q]["nb"] for q in range(q0, q0 + nq)], axis=1).reshape(-1, 3, 3)
    shifts = np.stack([c["shifts"] for c in cs], axis=1)
    return dict(peaks=np.ascontiguousarray(peaks), nb=np.ascontiguousarray(nb), shifts=np.ascontiguousarray(shifts),
                ref=cs[0]["ref"], max_r=np.full(NPATCH, SENTINEL, dtype=F32))
