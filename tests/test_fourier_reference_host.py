"""Host checks of tests/fourier_reference.py -- the float64 definitions, the derived bounds and the case tables of
tests/test_fourier_kernels_float64.py -- without a GPU: the reference against a dense DFT written out bin by bin,
integer shifts against rolls, the exposure filter at its edges, the fp32 CPU oracle INSIDE the derived bound (the
bound is not too tight for honest fp32 arithmetic), the max / rms condition the per-pixel cap rests on, and
operation-by-operation fp32 evaluations of the angle and of the exposure weight within their own terms."""

import functools
import math

import numpy as np
import pytest
import torch

import fourier_reference as fr
import oracle
from oracle import thirdparty_semantics as tp

U, F32 = fr.U, np.float32


# ------------------------------------------------------------------ the reference itself


def _dense_shift(x, sy, sx):
    """The operation from DFT matrices, complex128, no library transform: X = F_h x F_w restricted to kx <= w / 2,
    times the ramp, inverse along y, then the real inverse along x as c2r defines it -- the DC and (even w) Nyquist
    bins contribute their REAL part once, every other bin twice the real part of its term."""
    h, w = x.shape
    nk = w // 2 + 1
    y, ky = np.arange(h), np.arange(h)
    xs, kx = np.arange(w), np.arange(nk)
    X = np.exp(-2j * np.pi * np.outer(ky, y) / h) @ x.astype(np.complex128) @ np.exp(-2j * np.pi * np.outer(xs, kx) / w)
    fy = np.where(ky < (h + 1) // 2, ky, ky - h) / h
    fx = kx / w
    Z = X * np.exp(-2j * np.pi * (fy[:, None] * sy + fx[None, :] * sx))
    Zy = np.exp(2j * np.pi * np.outer(y, ky) / h) @ Z / h  # (h, nk)
    out = np.zeros((h, w))
    for k in range(nk):
        term = (Zy[:, k, None] * np.exp(2j * np.pi * k * xs / w)[None, :]).real
        once = k == 0 or (w % 2 == 0 and k == w // 2)
        out += term if once else 2 * term
    return out / w


@pytest.mark.parametrize("h,w", [(12, 10), (15, 16), (16, 15), (15, 17)])
def test_reference_is_the_dense_dft(h, w):
    """Also a half-integer shift on the even sizes: the Nyquist bin is multiplied by a complex value and only its
    real part (after the column transform) reaches the output."""
    rng = np.random.default_rng(h * 100 + w)
    x = rng.standard_normal((h, w))
    for sy, sx in [(0.0, 0.0), (0.5, -2.5), (-1.5, 0.5), (1.37, -2.81), (4.3, 0.0), (0.0, -5.7), (-20.25, 18.5)]:
        got = fr.fourier_shift64(x[None], [(sy, sx)])[0].numpy()
        assert np.abs(got - _dense_shift(x, sy, sx)).max() <= 1e-12, (h, w, sy, sx)


@pytest.mark.parametrize("h,w", [(12, 10), (15, 16), (16, 15), (15, 17), (64, 48)])
def test_integer_shifts_are_rolls_and_zero_is_the_identity(h, w):
    x = torch.from_numpy(np.random.default_rng(h + w).standard_normal((3, h, w)))
    got = fr.fourier_shift64(x, [(0, 0), (3, -7), (-5, 2)])
    assert float((got[0] - x[0]).abs().max()) <= 1e-12
    assert float((got[1] - torch.roll(x[1], shifts=(3, -7), dims=(0, 1))).abs().max()) <= 1e-12
    assert float((got[2] - torch.roll(x[2], shifts=(-5, 2), dims=(0, 1))).abs().max()) <= 1e-12


def test_one_axis_shifts_move_that_axis_only():
    """A non-square frame shifted along one axis: rows (or columns) are resampled, the other axis is untouched --
    swapped axes or a wrong sign of fy above h / 2 cannot pass (a fractional shift is checked through its
    composition with its complement to an integer; odd sizes, where no Nyquist bin loses its imaginary part)."""
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((1, 15, 23)))
    a = fr.fourier_shift64(fr.fourier_shift64(x, [(4.3, 0.0)]), [(0.7, 0.0)])
    assert float((a[0] - torch.roll(x[0], 5, 0)).abs().max()) <= 1e-12
    b = fr.fourier_shift64(fr.fourier_shift64(x, [(0.0, -5.7)]), [(0.0, -0.3)])
    assert float((b[0] - torch.roll(x[0], -6, 1)).abs().max()) <= 1e-12


def test_sign_convention_is_the_oracles():
    x = fr.case_frames(2, 16, 24)
    s = np.array([(3.0, -7.0), (0.5, -2.5)], dtype=F32)
    got = oracle.correct_motion_fast(x, _field(s))
    assert float((got.double() - fr.fourier_shift64(x, s)).abs().max()) <= 1e-5


def _field(shifts):
    """(2, t, 1, 1) field that makes correct_motion_fast apply `shifts` (it shifts by -field; a fresh tensor, the
    oracle negates it in place)."""
    return (-torch.from_numpy(np.asarray(shifts, dtype=F32))).t()[:, :, None, None].contiguous()


# ------------------------------------------------------------------ the exposure filter


def test_exposure_weights_at_their_edges():
    t, h, w = 4, 12, 10
    for ps, dose, pre, kv in fr.EXPOSURES + [(1.0, 1.0, 0.0, 199.0), (1.0, 1.0, 0.0, 200.0), (1.0, 1.0, 0.0, 299.9)]:
        wts = fr.exposure_weights64(t, h, w, ps, pre, dose, kv)
        assert wts.shape == (t, h, w // 2 + 1)
        assert float(((wts * wts).sum(0) - 1).abs().max()) <= 1e-14  # the normalisation
        # written out again with plain Python floats at a few bins
        scale = 1.0 if kv >= 300 else 0.8 if kv >= 200 else 0.75
        for ky, kx in [(0, 0), (1, 0), (0, 1), (h // 2, w // 2), (h - 1, 3), (7, 5)]:
            fy = (ky if ky < (h + 1) // 2 else ky - h) / h
            k = max(math.hypot(fy, kx / w) / ps, 1e-6)
            nc = (0.24499 * k ** -1.6649 + 2.8141) * scale
            q = [math.exp(-0.5 * (pre + dose * (f + 1)) / nc) for f in range(t)]
            n = math.sqrt(sum(v * v for v in q))
            for f in range(t):
                assert abs(float(wts[f, ky, kx]) - q[f] / n) <= 1e-14
    # DC: the clamp at 1e-6 makes N_c ~ 2.4e9, q = 1 to 1e-9, every frame weighs 1 / sqrt(t)
    assert float((fr.exposure_weights64(4, 12, 10, 1.0, 2.0, 1.5, 300.0)[:, 0, 0] - 0.5).abs().max()) <= 1e-8
    # voltage steps: N_c scales by 1 / 0.8 / 0.75, so E at 300 kV = 0.8 E at 200 kV = 0.75 E at 199 kV
    E300, _ = fr.exposure_exponents64(2, 8, 8, 1.1, 0.0, 1.0, 300.0)
    E200, _ = fr.exposure_exponents64(2, 8, 8, 1.1, 0.0, 1.0, 200.0)
    E199, _ = fr.exposure_exponents64(2, 8, 8, 1.1, 0.0, 1.0, 199.0)
    assert torch.allclose(E300, 0.8 * E200, rtol=1e-14) and torch.allclose(E300, 0.75 * E199, rtol=1e-14)
    assert fr.voltage_scale(300) == 1.0 and fr.voltage_scale(299.99) == 0.8 and fr.voltage_scale(200) == 0.8
    assert fr.voltage_scale(199.99) == 0.75
    # pre-exposure adds to every frame's dose: pre = 2 with dose 1 is frames 3, 4 of pre = 0
    Ep, _ = fr.exposure_exponents64(2, 8, 8, 1.0, 2.0, 1.0, 300.0)
    E0, _ = fr.exposure_exponents64(4, 8, 8, 1.0, 0.0, 1.0, 300.0)
    assert torch.allclose(Ep, E0[2:], rtol=1e-14)
    # one frame: q / sqrt(q^2) = 1 everywhere
    assert float((fr.exposure_weights64(1, 12, 10, 1.3, 2.0, 0.8, 200.0) - 1).abs().max()) <= 1e-15
    # against the oracle's fp32 filter
    for ps, dose, pre, kv in fr.EXPOSURES:
        ones = torch.ones(3, 16, 11, dtype=torch.complex64)
        got = tp.dose_weight_movie(ones, (16, 20), ps, pre, dose, kv).real.double()
        assert float((got - fr.exposure_weights64(3, 16, 20, ps, pre, dose, kv)).abs().max()) <= 1e-5


def test_shift_sums_are_the_definition():
    """shift_sums64 frame by frame against one more independent composition at a small odd size."""
    t, h, w = 3, 15, 16
    x = fr.case_frames(t, h, w, True)
    s = fr.case_shifts(t)[3:6]
    ps, dose, pre, kv = fr.EXPOSURES[1]
    res = fr.shift_sums64(x, s, ps, pre, dose, kv)
    y = torch.stack([torch.from_numpy(_dense_shift(x[f].double().numpy(), float(s[f, 0]), float(s[f, 1])))
                     for f in range(t)])
    assert float((res["plain"] - y.sum(0)).abs().max()) <= 1e-11
    wts = fr.exposure_weights64(t, h, w, ps, pre, dose, kv)
    dw = torch.fft.irfft2((wts * torch.fft.rfft2(y)), s=(h, w)).sum(0)
    assert float((res["dw"] - dw).abs().max()) <= 1e-11
    assert np.allclose(res["norm_y"], [float(torch.linalg.norm(y[f])) for f in range(t)], rtol=1e-12)


# ------------------------------------------------------------------ the tables


ALL_SHIFT_CASES = sorted({c[:4] for c in fr.ROW_MAJOR_SHIFT} | {c[:4] for c in fr.FUSED} | {c[:4] for c in fr.PRUNED}
                         | {c[:4] for c in fr.POLYPHASE} | {(*fr.FP16, True)})


def _layouts(case):
    """The kernel layouts a table case runs in."""
    out = []
    if case in {c[:4] for c in fr.ROW_MAJOR_SHIFT} | {c[:4] for c in fr.FUSED} | {(*fr.FP16, True)}:
        out.append("row_major")
    out += [c[5] for c in fr.PRUNED if c[:4] == case and c[4]]
    if case in {c[:4] for c in fr.POLYPHASE}:
        out.append("polyphase")
    return sorted(set(out))


def test_tables_hold_what_the_issue_lists():
    rows = {tuple(float(v) for v in r) for r in fr.case_shifts(1)}
    for want in fr.SHIFT_ROWS:
        assert tuple(float(F32(v)) for v in want) in rows
    for t in (1, 2, 3, 4, 5):
        sh = fr.case_shifts(t)
        assert len(sh) % t == 0 and len(sh) >= len(fr.SHIFT_ROWS) and np.abs(sh[len(fr.SHIFT_ROWS):]).max(initial=0) <= 3
    s = fr.case_shifts(1)
    assert ((s[:, 0] != 0) & (s[:, 1] == 0)).any() and ((s[:, 0] == 0) & (s[:, 1] != 0)).any()  # one axis only
    assert (np.abs(s - np.floor(s)) == 0.5).all(axis=1).any()  # half-integers on both axes
    assert float(np.abs(s).sum(1).max()) * math.pi > 1.1e3  # about 1.2e3 rad
    assert {c[1] for c in fr.ROW_MAJOR_SHIFT} >= {256, 512, 1024, 2048, 4096, 4092, 8184}
    assert {c[2] for c in fr.ROW_MAJOR_SHIFT} >= {64, 1024, 8192, 5760, 11520}
    assert len(fr.EXPOSURES) == 3 and {e[3] for e in fr.EXPOSURES} == {300.0, 200.0, 120.0}


@functools.lru_cache(maxsize=None)
def _oracle_errors(case):
    """Per shift row of a table case: (L2 error / ||ref||, max / rms of the error) of the fp32 CPU oracle against
    fourier_shift64, and the rows themselves."""
    t, h, w, offset = case
    out = []
    for launch in range(fr.launches(t)):
        x, s, ref = fr.shifted_reference(t, h, w, offset, launch)
        got = oracle.correct_motion_fast(x, _field(s))
        for f in range(t):
            l2, mx, rms = fr.measure(got[f], ref[f])
            out.append((tuple(float(v) for v in s[f]), l2 / float(torch.linalg.norm(ref[f])), mx / rms))
    return out


@pytest.mark.parametrize("case", ALL_SHIFT_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_fp32_oracle_lies_inside_the_bound_and_its_error_is_noise_like(case):
    """Honest fp32 arithmetic (torch's pocketfft, libm's sine and cosine) stays inside the derived bound -- the
    bound with the transform's pass list and the sin / cos term set to the oracle's -- on every case of the tables,
    and its error has max / rms <= 8: the condition under which a per-pixel cap of 10 rms bounds is no tighter
    than the L2 bound.  Prints the oracle's error over the KERNEL bound of each layout the case runs in."""
    t, h, w, offset = case
    errs = _oracle_errors(case)
    shifts = np.array([e[0] for e in errs])
    own = fr.bounds(h, w, shifts, "pocketfft", sincos=fr.SINCOS_LIBM)["rel"]
    for (s, rel, ratio), b in zip(errs, own):
        assert rel <= b, (case, s, rel, b)
        assert ratio <= fr.MAX_OVER_RMS, (case, s, ratio)
    worst = max(e[1] / b for e, b in zip(errs, own))
    line = f"ORACLE {case}: error / own bound {worst:.3f}, max/rms {max(e[2] for e in errs):.2f}"
    for layout in _layouts(case):
        kb = fr.bounds(h, w, shifts, layout)["rel"]
        line += f", / {layout} bound L2 {max(e[1] / b for e, b in zip(errs, kb)):.3f}" \
                f" pixel {max(e[1] * e[2] / (fr.CAP * b) for e, b in zip(errs, kb)):.3f}"
    print(line)


@pytest.mark.parametrize("case", [c for c in fr.FUSED if c[1] * c[2] <= 1 << 19] + [(3, 121, 135, False, False)],
                         ids=lambda c: "x".join(str(v) for v in c[:3]))
def test_fp32_oracle_sums_lie_inside_the_bound(case):
    """oracle.correct_motion_fast -> .sum(0) / oracle.dose_weighted_sum against shift_sums64.  The oracle's
    exposure-weighted sum transforms its own fp32 shifted frames a second time, so its bound has the shifted frames'
    error (and their rounding to fp32, u) and one more transform round trip with the filter term."""
    t, h, w, offset = case[:4]
    for launch in range(fr.launches(t)):
        x, s, _ = fr.shifted_reference(t, h, w, offset, launch)
        cor = oracle.correct_motion_fast(x, _field(s))
        b = fr.bounds(h, w, s, "pocketfft", sincos=fr.SINCOS_LIBM)
        for ps, dose, pre, kv in fr.EXPOSURES:
            ref = fr.shift_sums64(x, s, ps, pre, dose, kv)
            l2, mx, _ = fr.measure(cor.sum(0), ref["plain"])
            bound = fr.sum_l2_bound(b["rel"], ref["norm_y"])
            assert l2 <= bound and mx <= fr.CAP * bound / math.sqrt(h * w), (case, launch, l2, mx, bound)
            expo = fr.exposure_term(t, h, w, ps, pre, dose, kv)
            again = b["fft"] + expo + 2 * U
            bound = fr.sum_l2_bound(again, ref["norm_d"], extra=float(((b["rel"] + U) * ref["norm_y"]).sum()))
            l2, mx, _ = fr.measure(oracle.dose_weighted_sum(cor, ps, dose, pre, kv), ref["dw"])
            assert l2 <= bound and mx <= fr.CAP * bound / math.sqrt(h * w), (case, launch, (ps, dose, pre, kv), l2, bound)


# ------------------------------------------------------------------ the terms, operation by operation


def _f(x):
    return np.asarray(x, dtype=F32)


@pytest.mark.parametrize("h,w", [(256, 64), (4092, 64), (121, 135), (256, 5760), (8184, 128)])
def test_angle_term_bounds_an_fp32_evaluation(h, w):
    """(-2 pi fy) sy + (-2 pi fx) sx with every operation rounded to fp32, as the kernels and the oracle write it
    (fy = k * fp32(1 / h)), against the exact angle of the same fp32 shifts."""
    ky = np.arange(h)
    kk = np.where(ky < (h + 1) // 2, ky, ky - h)
    fy = _f(kk) * F32(1.0 / h)
    fx = _f(np.arange(w // 2 + 1)) * F32(1.0 / w)
    m2pi = F32(-6.283185307179586)
    for sy, sx in fr.case_shifts(1):
        ang = ((m2pi * fy) * sy)[:, None] + ((m2pi * fx) * sx)[None, :]
        assert ang.dtype == F32
        exact = -2 * np.pi * ((kk / h)[:, None] * float(sy) + (np.arange(w // 2 + 1) / w)[None, :] * float(sx))
        term = fr.angle_term([(sy, sx)])[0]
        assert np.abs(ang.astype(np.float64) - exact).max() <= term, (h, w, sy, sx)


@pytest.mark.parametrize("h,w", [(256, 256), (4092, 64), (121, 135)])
def test_exposure_term_bounds_an_fp32_evaluation(h, w):
    """The chain of csrc/full_sums.hip::full_dose_mh and the accumulation kernels in numpy fp32: k, powf, N_c,
    -0.5 / N_c, N_f, expf, sum of squares, root, quotient."""
    t = 5
    ky = np.arange(h)
    fy = _f(np.where(ky < (h + 1) // 2, ky, ky - h)) * F32(1.0 / h)
    fx = _f(np.arange(w // 2 + 1)) * F32(1.0 / w)
    for ps, dose, pre, kv in fr.EXPOSURES:
        k = np.maximum(np.sqrt(fy[:, None] * fy[:, None] + fx[None, :] * fx[None, :]) / F32(ps), F32(1e-6))
        ncrit = (F32(0.24499) * np.power(k, F32(-1.6649)) + F32(2.8141)) * F32(fr.voltage_scale(kv))
        mh = F32(-0.5) / ncrit
        q = np.stack([np.exp((F32(pre) + F32(dose) * F32(f + 1)) * mh) for f in range(t)])
        wts = q / np.sqrt((q * q).sum(0, dtype=F32))
        assert wts.dtype == F32
        ref = fr.exposure_weights64(t, h, w, ps, pre, dose, kv).numpy()
        rel = np.abs(wts.astype(np.float64) - ref) / ref
        term = fr.exposure_term(t, h, w, ps, pre, dose, kv)
        assert (rel.max(axis=(1, 2)) <= term).all(), (h, w, ps, rel.max(axis=(1, 2)), term)


def test_transform_costs_follow_the_plans():
    """Pass lists and line kinds the FFT term is built from."""
    from torch_motion_correction_amd import plan

    assert fr.smooth_radix_list(4092) == [31, 11, 12] and fr.smooth_radix_list(8184) == [31, 11, 24]
    assert fr.smooth_radix_list(2880) == [8, 8, 9, 5] and fr.smooth_radix_list(5760) == [8, 8, 9, 10]
    assert abs(fr.ETA / U - 6.66) < 0.01 and abs(fr.radix_cost(16) - 4 * fr.ETA) < 1e-20
    c, _ = fr.transform_cost(256, 256, "row_major")
    assert abs(c - 2 * (8 + 8) * fr.ETA) < 1e-12  # 2 (log2 h + log2 w) eta
    try:
        for case in fr.PRUNED:
            plan.USE_DIRECT_LINES = case[4]
            plan._LINES.clear()
            _, kinds = fr.transform_cost(case[1], case[2], case[5])
            assert (kinds["rows"], kinds["cols"]) == case[6], (case, kinds)
    finally:
        plan.USE_DIRECT_LINES = True
        plan._LINES.clear()
    with pytest.raises(NotImplementedError):
        plan.full_geometry(96, 7000)
