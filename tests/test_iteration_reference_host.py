"""Host checks of tests/iteration_reference.py (no GPU): the float64 definitions mean what the package uses them for,
an fp32 numpy stand-in written in the kernels' order of operations lies inside every derived bound on every shared case
(its worst error / bound per output family is printed: the host ratios of DESIGN.md section 6), every comparison
rejects its deliberately wrong stand-in, and the C entry points answer MC_ERR_ARG before any launch."""

import ctypes
import math

import numpy as np
import pytest
import torch

import global_refine_reference as grr
import iteration_reference as ir
from kernel_harness import ratios_fixture, worse
from oracle.local_motion import compute_loss

F32, U = np.float32, ir.U


# ------------------------------------------------------------------ the definitions mean what the package uses them for


def _patch_spectra(npatch, t, ph, pw, seed):
    """Half spectra (npatch, t, ph, pw // 2 + 1) of real patches, rounded to fp32, with what the package's band-pass
    removes set to zero: DC, and the Nyquist row and column of an even side (a fractional shift of those is not the
    spectrum of a real patch)."""
    r = np.random.default_rng([seed, t, ph, pw])
    P = np.fft.rfft2(r.normal(0, 1, (npatch, t, ph, pw)))
    P[..., 0, 0] = 0
    if ph % 2 == 0:
        P[..., ph // 2, :] = 0
    if pw % 2 == 0:
        P[..., :, pw // 2] = 0
    return P.astype(np.complex64)


@pytest.mark.parametrize("loss_type", ["mse", "cc", "ncc"])
@pytest.mark.parametrize("t", [2, 5])
@pytest.mark.parametrize("shape", [(12, 10), (9, 11)])
def test_float64_sums_give_the_spatial_domain_loss_and_its_gradient(loss_type, t, shape):
    from torch_motion_correction_amd.local_motion import LocalMotionProblem

    ph, pw = shape
    npatch, nkx = 2, pw // 2 + 1
    P = _patch_spectra(npatch, t, ph, pw, 1)
    fy = np.fft.fftfreq(ph).astype(F32)
    fx = (np.arange(nkx) / pw).astype(F32)
    kx = np.arange(nkx)
    hx = np.where((kx == 0) | ((pw % 2 == 0) & (kx == pw // 2)), 1.0, 2.0).astype(F32)
    shifts = np.random.default_rng([2, t, ph]).uniform(-2, 2, (npatch, t, 2)).astype(F32)
    wb = torch.tensor([0.625, 0.375], dtype=torch.float64)
    Pk = np.ascontiguousarray(P.transpose(0, 1, 3, 2))  # the kernels' layout: (npatch, t, nkx, nky)

    prob = object.__new__(LocalMotionProblem)  # loss_and_grad itself, its two kernel calls answered in float64
    prob.t, prob.ph, prob.pw = t, ph, pw
    prob.sums = lambda s, hermitian: torch.from_numpy(ir.loss_sums64(Pk, s.numpy(), fy, fx, hx if hermitian else None))
    prob.ncc_grad_sums = lambda s, ab: torch.from_numpy(ir.ncc_grad_sums64(Pk, s.numpy(), fy, fx, hx, ab.numpy()))
    loss, grad = prob.loss_and_grad(torch.from_numpy(shifts.astype(np.float64)), wb, loss_type)

    s = torch.from_numpy(shifts.astype(np.float64)).requires_grad_(True)
    ang = torch.from_numpy(fy.astype(np.float64))[None, None, :, None] * s[:, :, 0, None, None] \
        + torch.from_numpy(fx.astype(np.float64))[None, None, None, :] * s[:, :, 1, None, None]
    G = torch.from_numpy(P.astype(np.complex128)) * torch.polar(torch.ones_like(ang), -2 * math.pi * ang)
    R = (G.sum(dim=1, keepdim=True) - G) / (t - 1)
    want = sum(wb[b] * compute_loss(G[b], R[b], ph, pw, loss_type) for b in range(npatch))
    (gwant,) = torch.autograd.grad(want, s)
    assert want.dtype == torch.float64
    assert abs(float(loss) - float(want)) <= 1e-10 * abs(float(want)), (float(loss), float(want))
    assert float((grad - gwant).abs().max()) <= 1e-10 * float(gwant.abs().max())
    assert float(gwant.abs().max()) > 0


@pytest.mark.parametrize("shape", [(12, 10), (9, 11)])
def test_aligned_refs_translate_the_true_correlation_map_by_under(shape):
    H, W = shape
    t, under = 3, 2
    S = np.fft.rfft2(np.random.default_rng([3, H, W]).normal(0, 1, (t, H, W))).astype(np.complex64)
    Sk = S.transpose(0, 2, 1)  # (t, nkx, nky)
    s = np.array([[0.3, -1.2], [2.0, 0.75], [-0.6, 1.0]], dtype=F32)
    fy, fx = np.fft.fftfreq(H), np.fft.rfftfreq(W)
    cmap = lambda G, R: np.fft.irfft2((np.conj(R) * G).transpose(0, 2, 1), s=(H, W))
    true = cmap(*ir.aligned_refs64(Sk, s, fy, fx, 0))
    got = cmap(*ir.aligned_refs64(Sk, s, fy, fx, under))
    assert np.abs(got - np.roll(true, (under, under), (1, 2))).max() <= 1e-12 * np.abs(true).max()


def test_refine_update64_reproduces_an_iteration_of_the_restated_estimator():
    t, h, w, under = 4, 32, 40, 4
    movie, _ = grr.planted_movie(t, h, w, [0, 0.3, -0.6, 1.2], [0, -0.4, 0.7, 0.2], noise=0.1)
    S = grr.filtered_spectra(movie, 1.0)
    ref = t // 2
    s0 = grr.integer_shifts(S, (h, w), ref)
    s1, hist, offs = grr.refine_shifts(S, (h, w), ref, start=s0, max_iterations=1)
    G, R = ir.aligned_refs64(S.transpose(0, 2, 1), s0, np.fft.fftfreq(h), np.fft.rfftfreq(w), under)
    cc = np.fft.irfft2((np.conj(R) * G).transpose(0, 2, 1), s=(h, w))
    peaks = cc.reshape(t, -1).argmax(axis=1)
    nb = np.empty((t, 3, 3))
    for f in range(t):
        py, px = divmod(int(peaks[f]), w)
        for i in range(3):
            for j in range(3):
                nb[f, i, j] = cc[f, (py + i - 1) % h, (px + j - 1) % w]
    got, max_r, _, _, r, off = ir.refine_update64(peaks, nb, s0, ref, h, w, under, damp=(t - 1) / t, bounds=True)
    assert np.abs(off - offs[0]).max() <= 1e-9 and np.abs(offs[0]).max() > 0.05
    assert np.abs(got - s1).max() <= 1e-9 and abs(max_r - hist[0]) <= 1e-9
    assert not got[ref].any()


# ------------------------------------------------------------------ the fp32 stand-in, in the kernels' order


def _sincospi32(x):
    x = x.astype(np.float64)
    return np.sin(np.pi * x).astype(F32), np.cos(np.pi * x).astype(F32)


def _lane_sum(terms, nt):
    """(npatch, nt * 1024) fp32 -> (npatch, nt): 16 sequential additions per lane, then the xor butterfly."""
    v = terms.reshape(terms.shape[0], nt, 16, 64)
    acc = np.zeros_like(v[:, :, 0])
    for i in range(16):
        acc = acc + v[:, :, i]
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lane ^ o]
    return acc[:, :, 0]


def loss_standin(c, hx, mode, fault=None):
    """local_loss_kernel<mode> in numpy fp32 -> (npatch, ntiles, t, 6 or 2)."""
    P = c["P"]
    npatch, t, nkx, nky, _ = P.shape
    nbins, nt = nkx * nky, ir.ntiles(nkx, nky)
    pos = np.arange(nt * ir.LM_TILE)
    k = pos - (pos >= ir.LM_TILE) if fault == "tile base" else pos
    valid = k < nbins
    kc = np.minimum(k, nbins - 1)
    kx, ky = kc // nky, kc % nky
    Pf = P.reshape(npatch, t, nbins, 2)[:, :, kc]
    fyk, fxk = c["fy"][ky], c["fx"][kx]
    hk = np.ones(len(pos), dtype=F32) if hx is None else (hx[ky % nkx] if fault == "hx by ky" else hx[kx])
    two = F32(2.0 if fault == "conjugated phase" else -2.0)
    sh, ab = c["shifts"], c["ab"]
    inv = F32(1) / F32(t if fault == "1/t" else max(t - 1, 1))

    def g(f):
        s, co = _sincospi32(two * (fyk * sh[:, f, 0, None] + fxk * sh[:, f, 1, None]))
        px, py = Pf[:, f, :, 0], Pf[:, f, :, 1]
        return px * co - py * s, px * s + py * co

    Sx = Sy = np.zeros((npatch, len(pos)), dtype=F32)
    for f in range(t):
        gx, gy = g(f)
        Sx, Sy = Sx + gx, Sy + gy
    if mode == 1:
        Cx = Cy = np.zeros_like(Sx)
        for f in range(t - 1 if fault == "C without the last frame" else t):
            gx, gy = g(f)
            af, bf = ab[:, f, 0, None], F32(2) * ab[:, f, 1, None] * inv
            Cx = Cx + (af * gx + bf * (Sx - gx))
            Cy = Cy - (af * gy + bf * (Sy - gy))
    out = np.zeros((npatch, nt, t, 6 if mode == 0 else 2), dtype=F32)
    tf = F32(t - 1 if fault == "(t-1) G - S" else t)
    for f in range(t):
        gx, gy = g(f)
        if mode == 0:
            im = Sx * gy - Sy * gx
            dx, dy = tf * gx - Sx, tf * gy - Sy
            rx, ry = Sx - gx, Sy - gy
            terms = [hk * fyk * im, hk * fxk * im, hk * (dx * dx + dy * dy), hk * (gx * rx + gy * ry),
                     hk * (rx * rx + ry * ry), hk * (gx * gx + gy * gy)]
        else:
            af, bf = ab[:, f, 0, None], F32(2) * ab[:, f, 1, None] * inv
            rx, ry = (Sx - gx) * inv, (Sy - gy) * inv
            cfx, cfy = af * gx + bf * (Sx - gx), -(af * gy + bf * (Sy - gy))
            vx, vy = af * rx + (Cx - cfx) * inv, -af * ry + (Cy - cfy) * inv
            im = vx * gy + vy * gx
            terms = [hk * fyk * im, hk * fxk * im]
        for ci, term in enumerate(terms):
            assert term.dtype == F32
            out[:, :, f, ci] = _lane_sum(np.where(valid, term, F32(0)), nt)
    if fault == "last tile dropped":
        out[:, -1] = 0
    return out


def _cis32(rev):
    r = (rev - np.floor(rev)).astype(np.float64)
    return np.cos(2 * np.pi * r).astype(F32), np.sin(2 * np.pi * r).astype(F32)


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _cmul32(a, b):
    return _fma32(-a[1], b[1], a[0] * b[0]), _fma32(a[1], b[0], a[0] * b[1])


def aligned_standin(S, shifts, offsets, fy, fx, under, q0, nq, fault=None):
    """xc_aligned_refs_patches in numpy fp32: S (t, npatch, nkx, nky, 2) -> (G', REF) (t, nq, nkx, nky, 2).  The plain
    kernel is npatch = 1 with zero offsets (s - 0 is s)."""
    t, npatch, nkx, nky, _ = S.shape
    slots = npatch if fault == "written at q" else nq
    G = np.full((t, slots, nkx, nky, 2), np.nan, dtype=F32)
    REF = np.full((t, slots, nkx, nky, 2), np.nan, dtype=F32)
    fyb, fxb = np.asarray(fy, dtype=F32)[None, :], np.asarray(fx, dtype=F32)[:, None]
    un = F32(under)
    E = _cmul32(_cis32(-(fyb * un) + np.zeros((nkx, nky), dtype=F32)), _cis32(-(fxb * un) + np.zeros((nkx, nky), dtype=F32)))
    inv = F32(1) / F32(t - 1) if t > 1 else F32(0)
    for qc in range(nq):
        q = q0 + qc

        def g(f):
            dy, dx = shifts[f, q, 0] - offsets[f, q, 0], shifts[f, q, 1] - offsets[f, q, 1]
            ramp = _cmul32(_cis32(fyb * dy + np.zeros((nkx, nky), dtype=F32)), _cis32(fxb * dx + np.zeros((nkx, nky), dtype=F32)))
            return _cmul32((S[f, q, :, :, 0], S[f, q, :, :, 1]), ramp)

        Ax = Ay = np.zeros((nkx, nky), dtype=F32)
        for f in range(t):
            gx, gy = g(f)
            Ax, Ay = Ax + gx, Ay + gy
        slot = q if fault == "written at q" else qc
        for f in range(t):
            gv = g(f)
            G[f, slot, :, :, 0], G[f, slot, :, :, 1] = _cmul32(gv, E)
            REF[f, slot, :, :, 0], REF[f, slot, :, :, 1] = (Ax - gv[0]) * inv, (Ay - gv[1]) * inv
    return G[:, :nq], REF[:, :nq]


def update_standin(peaks, nb, shifts, ref, H, W, under, fault=None):
    """xc_refine_update in numpy fp32 -> (shifts (t, 2) fp32, max_r fp32)."""
    pk = np.asarray(peaks, dtype=np.int64)
    t = len(pk)
    nb = np.asarray(nb, dtype=F32).reshape(t, 3, 3)
    r = np.zeros((t, 2), dtype=F32)
    for c, (n, i, (v0, v1, v2)) in enumerate(((H, pk // W, (nb[:, 0, 1], nb[:, 1, 1], nb[:, 2, 1])),
                                              (W, pk % W, (nb[:, 1, 0], nb[:, 1, 1], nb[:, 1, 2])))):
        i = i - under
        i = np.where(i < 0, i + n, i)
        keep = (i < n // 2) if fault == "wrap with <" else (i <= n // 2)
        ri = np.where(keep, i, i - n).astype(F32)
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = (v0 == v0) & (v2 == v2) & (v2 != v0)
            off = (F32(0.5) * (v0 - v2)) / ((v0 - F32(2) * v1) + v2)
        r[:, c] = np.where(ok, ri + np.where(ok, off, F32(0)), ri)
    damp = F32(t - 1) / F32(t)
    s = np.asarray(shifts, dtype=F32).reshape(t, 2)
    s1 = s + damp * r
    sref = s[ref] if fault == "sref from before the update" else s1[ref]
    new = s1 - sref
    new[ref] = 0
    m = np.abs(r[:64] if fault == "max_r over wave 0" else r).max()
    assert new.dtype == F32
    return new, F32(m)


def update_patches_standin(c, q0, nq, H, W, under):
    s, mr = c["shifts"].copy(), c["max_r"].copy()
    t = s.shape[0]
    pk, nb = c["peaks"].reshape(t, nq), c["nb"].reshape(t, nq, 3, 3)
    for qc in range(nq):
        s[:, q0 + qc], mr[q0 + qc] = update_standin(pk[:, qc], nb[:, qc], s[:, q0 + qc], c["ref"], H, W, under)
    return s, mr


# ------------------------------------------------------------------ the stand-in inside every bound, every shared case


ratios = ratios_fixture("RATIO fp32 stand-in")


@pytest.mark.parametrize("case", ir.LOSS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_loss_standin_within_bounds(ratios, case):
    for sf in ir.SHIFT_FORMS:
        c = ir.loss_case(case, sf)
        for hf in ir.HX_FORMS:
            hx = ir.make_hx(hf, case[2])
            ref, bound = ir.loss_tiles64(c["P"], c["shifts"], c["fy"], c["fx"], hx)
            r = ir.assert_within(loss_standin(c, hx, 0), ref, bound, f"loss sums {case} {sf} {hf}")
            worse(ratios, "mc_local_loss_sums", r)
            ref, bound = ir.ncc_grad_tiles64(c["P"], c["shifts"], c["fy"], c["fx"], hx, c["ab"])
            r = ir.assert_within(loss_standin(c, hx, 1), ref, bound, f"ncc grad {case} {sf} {hf}")
            worse(ratios, "mc_local_ncc_grad", r)
            if sf == "aligned":  # the float64 q and d2 are at rounding level: far below the absolute bound's own size
                q = ir.loss_sums64(c["P"], c["shifts"], c["fy"], c["fx"], hx)
                assert np.abs(q[..., :3]).max() <= 1e-4 * max(np.abs(q[..., 5]).max(), 1e-30) * case[1] ** 2, (case, hf)


@pytest.mark.parametrize("case", ir.ALIGNED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_aligned_refs_standin_within_bounds(ratios, case):
    c = ir.aligned_case(case)
    zero = np.zeros((case[0], 1, 2), dtype=F32)
    G, REF = aligned_standin(c["S"][:, None], c["shifts"][:, None], zero, c["fy"], c["fx"], c["under"], 0, 1)
    rg, rr = ir.check_aligned(G[:, 0], REF[:, 0], ir.aligned_refs64(c["S"], c["shifts"], c["fy"], c["fx"], c["under"], True),
                              f"aligned refs {case}")
    worse(ratios, "mc_xc_aligned_refs G'", rg)
    worse(ratios, "mc_xc_aligned_refs REF", rr)
    p = ir.aligned_patch_case(case)
    for q0, nq in ir.PATCH_RANGES:
        G, REF = aligned_standin(p["S"], p["shifts"], p["offsets"], p["fy"], p["fx"], p["under"], q0, nq)
        ref4 = ir.aligned_refs_patches64(p["S"], p["shifts"], p["offsets"], p["fy"], p["fx"], p["under"], q0, nq, True)
        rg, rr = ir.check_aligned(G, REF, ref4, f"aligned refs patches {case} {(q0, nq)}")
        worse(ratios, "mc_xc_aligned_refs_patches G'", rg)
        worse(ratios, "mc_xc_aligned_refs_patches REF", rr)


def _update_cases():
    return [(t, v, shape, under) for t in ir.UPDATE_T for v in range(3) for shape, under in ir.UPDATE_SHAPES]


def test_update_inputs_have_known_denominators_and_hit_every_guard():
    kinds = set()
    for t, v, shape, under in _update_cases():
        c = ir.update_case(t, v, shape, under)
        ev, ok = ir.parabola_den_condition(c["nb"])
        assert ok.all(), (t, v, shape)  # |den| > 4E on every evaluated axis: the share left out is zero
        assert c["ref"] == ir.update_refs(t)[v] and c["big"] == (t - 1, 0, c["ref"])[v]
        r, _, _ = ir.residuals64(c["peaks"], c["nb"], *shape, under)
        assert np.abs(r[c["big"]]).max() == np.abs(r).max() and (np.abs(np.delete(r, c["big"], 0)) < np.abs(r).max() - 0.1).all()
        H, W = shape
        assert np.allclose(r[c["big"]], (H // 2 + 4 / 9, W // 2 + 4 / 9), atol=1e-6)  # the peak at exactly n / 2 stays +n / 2
        for f, k in enumerate(c["kinds"]):
            kinds.add(k)
            if k == "half+1":
                assert -(H - H // 2 - 1) <= r[f, 0] < -(H - H // 2 - 1) + 0.5 and -(W - W // 2 - 1) <= r[f, 1] < 0
            if k == "below":
                assert (r[f] < -0.4).all()
            if k in ("v0==v2", "flat"):
                assert not ev[f].any()
            if k == "nan-y":
                assert not ev[f, 0] and ev[f, 1]
            if k == "nan-x":
                assert ev[f, 0] and not ev[f, 1]
        for q0, nq in ir.PATCH_RANGES:
            assert ir.parabola_den_condition(ir.update_patch_case(t, v, shape, under, q0, nq)["nb"])[1].all()
    assert kinds == {"centre", "below", "half+1", "nan-y", "nan-x", "v0==v2", "flat", "plain", "big"}


def test_update_standin_within_bounds(ratios):
    for i, (t, v, shape, under) in enumerate(_update_cases()):
        c = ir.update_case(t, v, shape, under)
        ref4 = ir.refine_update64(c["peaks"], c["nb"], c["shifts"], c["ref"], *shape, under, bounds=True)
        rs, rm = ir.check_update(*update_standin(c["peaks"], c["nb"], c["shifts"], c["ref"], *shape, under), ref4, c["ref"],
                                 f"update {(t, v, shape)}")
        worse(ratios, "mc_xc_refine_update shifts", rs)
        worse(ratios, "mc_xc_refine_update max_r", rm)
        for q0, nq in ir.PATCH_RANGES:
            p = ir.update_patch_case(t, v, shape, under, q0, nq)
            ref4 = ir.refine_update_patches64(p["peaks"], p["nb"], p["shifts"], p["ref"], q0, nq, *shape, under, p["max_r"], True)
            s, mr = update_patches_standin(p, q0, nq, *shape, under)
            rs, rm = ir.check_update_patches(s, mr, p["shifts"], p["max_r"], ref4, p["ref"], q0, nq, f"update patches {(t, v, shape, q0, nq)}")
            worse(ratios, "mc_xc_refine_update_patches shifts", rs)
            worse(ratios, "mc_xc_refine_update_patches max_r", rm)


# ------------------------------------------------------------------ every comparison rejects its wrong stand-in


LOSS_FAULTS = [("tile base", (2, 4, 25, 41), 0), ("tile base", (2, 7, 33, 65), 1), ("last tile dropped", (2, 4, 25, 41), 0),
               ("last tile dropped", (2, 7, 33, 65), 1), ("hx by ky", (2, 5, 5, 9), 0), ("hx by ky", (2, 5, 5, 9), 1),
               ("conjugated phase", (2, 5, 5, 9), 0), ("conjugated phase", (2, 5, 5, 9), 1), ("1/t", (2, 5, 5, 9), 1),
               ("C without the last frame", (2, 5, 5, 9), 1), ("(t-1) G - S", (2, 5, 5, 9), 0)]


@pytest.mark.parametrize("fault,case,mode", LOSS_FAULTS, ids=lambda v: str(v).replace(" ", "_"))
def test_loss_comparison_rejects_the_wrong_standin(fault, case, mode):
    c = ir.loss_case(case, "random")
    hx = ir.make_hx("arbitrary", case[2])
    if mode == 0:
        ref, bound = ir.loss_tiles64(c["P"], c["shifts"], c["fy"], c["fx"], hx)
    else:
        ref, bound = ir.ncc_grad_tiles64(c["P"], c["shifts"], c["fy"], c["fx"], hx, c["ab"])
    ir.assert_within(loss_standin(c, hx, mode), ref, bound, "control")
    with pytest.raises(AssertionError, match="beyond the bound"):
        ir.assert_within(loss_standin(c, hx, mode, fault), ref, bound, fault)


def test_conjugated_phase_is_rejected_in_the_aligned_regime_too():
    """Where every sum cancels a relative tolerance says nothing; the absolute bound still tells +s from -s."""
    c = ir.loss_case((2, 5, 5, 9), "aligned")
    ref, bound = ir.loss_tiles64(c["P"], c["shifts"], c["fy"], c["fx"], None)
    ir.assert_within(loss_standin(c, None, 0), ref, bound, "control")
    with pytest.raises(AssertionError, match="beyond the bound"):
        ir.assert_within(loss_standin(c, None, 0, "conjugated phase"), ref, bound, "conjugated")


def test_update_comparison_rejects_the_wrong_standins():
    shape, under = ir.UPDATE_SHAPES[0]
    for fault, t, v in (("max_r over wave 0", 65, 0), ("max_r over wave 0", 130, 2), ("sref from before the update", 65, 0),
                        ("sref from before the update", 6, 1), ("wrap with <", 6, 0), ("wrap with <", 130, 1)):
        c = ir.update_case(t, v, shape, under)
        ref4 = ir.refine_update64(c["peaks"], c["nb"], c["shifts"], c["ref"], *shape, under, bounds=True)
        ir.check_update(*update_standin(c["peaks"], c["nb"], c["shifts"], c["ref"], *shape, under), ref4, c["ref"], "control")
        with pytest.raises(AssertionError, match="beyond the bound"):
            ir.check_update(*update_standin(c["peaks"], c["nb"], c["shifts"], c["ref"], *shape, under, fault), ref4, c["ref"], fault)


def test_patch_comparison_rejects_output_written_at_q():
    case = (6, 5, 9, 16)
    p = ir.aligned_patch_case(case)
    for q0, nq in ((2, 2), (4, 1)):
        ref4 = ir.aligned_refs_patches64(p["S"], p["shifts"], p["offsets"], p["fy"], p["fx"], p["under"], q0, nq, True)
        args = (p["S"], p["shifts"], p["offsets"], p["fy"], p["fx"], p["under"], q0, nq)
        ir.check_aligned(*aligned_standin(*args), ref4, "control")
        with pytest.raises(AssertionError, match="beyond the bound"):
            ir.check_aligned(*aligned_standin(*args, fault="written at q"), ref4, "written at q")


# ------------------------------------------------------------------ the C entry points validate before they launch


def _p(i):
    return ctypes.c_void_p(0x100000 * (i + 1))


def test_entry_points_answer_err_arg_before_any_launch():
    """Fake pointers and a null stream: every call below must answer MC_ERR_ARG (-1) before it launches anything."""
    from torch_motion_correction_amd import _lib

    lib = _lib.load()

    def sums(P=_p(0), sh=_p(1), fy=_p(2), fx=_p(3), hx=_p(4), npatch=2, t=5, nkx=5, nky=9, out=_p(5)):
        return lib.mc_local_loss_sums(P, sh, fy, fx, hx, npatch, t, nkx, nky, out, None)

    def grad(P=_p(0), sh=_p(1), fy=_p(2), fx=_p(3), hx=_p(4), ab=_p(6), npatch=2, t=5, nkx=5, nky=9, out=_p(5)):
        return lib.mc_local_ncc_grad(P, sh, fy, fx, hx, ab, npatch, t, nkx, nky, out, None)

    for fn, names in ((sums, ("P", "sh", "fy", "fx", "out")), (grad, ("P", "sh", "fy", "fx", "ab", "out"))):
        for name in names:
            assert fn(**{name: None}) == -1, name
        assert fn(t=0) == -1 and fn(t=513) == -1 and fn(npatch=0) == -1 and fn(npatch=65536) == -1
        assert fn(nkx=0) == -1 and fn(nky=0) == -1
        assert fn(nkx=1 << 16, nky=1 << 16) == -1      # nkx * nky wraps to 0 in an int
        assert fn(nkx=1 << 15, nky=1 << 16) == -1      # 2^31: beyond an int bin index
        assert fn(nkx=46341, nky=46341) == -1          # 2147488281 wraps negative
    nt = ctypes.c_int(-5)
    assert lib.mc_local_loss_tiles(1 << 16, 1 << 16, ctypes.byref(nt)) == -1 and nt.value == -5
    assert lib.mc_local_loss_tiles(5, 9, None) == -1 and lib.mc_local_loss_tiles(0, 9, ctypes.byref(nt)) == -1
    assert lib.mc_local_loss_tiles(33, 65, ctypes.byref(nt)) == 0 and nt.value == 3
    assert lib.mc_local_loss_tiles(16, 64, ctypes.byref(nt)) == 0 and nt.value == 1
    assert lib.mc_local_loss_tiles(46340, 46340, ctypes.byref(nt)) == 0 and nt.value == ir.ntiles(46340, 46340)

    def refs(S=_p(0), sh=_p(1), fy=_p(2), fx=_p(3), G=_p(4), REF=_p(5), t=6, nkx=5, nky=9, under=16):
        return lib.mc_xc_aligned_refs(S, sh, fy, fx, G, REF, t, nkx, nky, under, None)

    for name in ("S", "sh", "fy", "fx", "G", "REF"):
        assert refs(**{name: None}) == -1, name
    assert refs(t=0) == -1 and refs(t=513) == -1 and refs(nkx=0) == -1 and refs(nky=0) == -1 and refs(under=-1) == -1

    def upd(peaks=_p(0), nb=_p(1), sh=_p(2), ref=3, t=6, H=96, W=120, under=16, mx=_p(3)):
        return lib.mc_xc_refine_update(peaks, nb, sh, ref, t, H, W, under, mx, None)

    for name in ("peaks", "nb", "sh", "mx"):
        assert upd(**{name: None}) == -1, name
    assert upd(t=0) == -1 and upd(t=1) == -1 and upd(t=513) == -1 and upd(ref=-1) == -1 and upd(ref=6) == -1
    assert upd(H=1) == -1 and upd(W=1) == -1 and upd(under=-1) == -1 and upd(under=96) == -1

    def prefs(S=_p(0), sh=_p(1), of=_p(2), fy=_p(3), fx=_p(4), G=_p(5), REF=_p(6), t=6, npatch=5, q0=0, nq=5, nkx=5, nky=9,
              under=16):
        return lib.mc_xc_aligned_refs_patches(S, sh, of, fy, fx, G, REF, t, npatch, q0, nq, nkx, nky, under, None)

    assert prefs(S=None) == -1 and prefs(t=0) == -1 and prefs(t=513) == -1 and prefs(q0=4, nq=2) == -1
    assert prefs(npatch=70000, nq=65536) == -1 and prefs(nkx=1 << 16, nky=1 << 16) == -1

    def pupd(peaks=_p(0), nb=_p(1), sh=_p(2), ref=3, t=6, npatch=5, q0=0, nq=5, H=96, W=120, under=16, mx=_p(3)):
        return lib.mc_xc_refine_update_patches(peaks, nb, sh, ref, t, npatch, q0, nq, H, W, under, mx, None)

    assert pupd(peaks=None) == -1 and pupd(t=0) == -1 and pupd(t=513) == -1 and pupd(q0=4, nq=2) == -1 and pupd(ref=6) == -1
