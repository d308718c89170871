"""Every Fourier-shift and exposure-sum kernel against the float64 definitions of tests/fourier_reference.py
(fourier_shift64, exposure_weights64, shift_sums64): the row-major engine (csrc/full_fft.hip and full_sums.hip: row passes of 64 to
8192, 5760 and 11520 columns, column passes of 256 to 2048 rows, the radix-16 4096, the mixed-radix 4092 / 8184, the
fused shift-sum pass in its four modes, row-major and column-major fed, one chunk and several), the pruned engine in
its transposed layout (native, direct mixed-radix, chirp-z and odd unpacked lines; mc_dose_accumulate), the
x-polyphase form, the raw u8 / i16 row pass and an fp16 stack -- through the public API, at shifts from zero to
(-200.25, 180.5) px (about 1.2e3 rad), with no pixel excluded.  Every test asserts which entry points of libmcorr
ran (a recorder around the loaded library), so a silent fallback cannot pass as coverage.

Bounds (fourier_reference.bounds, derived rounding by rounding there; none is fitted to a kernel's output):

  frame  ||got - ref||_2 <= rel ||ref||_2, rel = fft + angle + sincos + ramp
           fft     Higham's log2(N) eta per power-of-two line (eta = 6.66 u, twiddles rounded from float64), the
                   pass list of the mixed-radix lines, and for chirp-z both M-point transforms and the three
                   pointwise products times the filter's amplification; forward and inverse, rows and columns
           angle   6 roundings of the fp32 angle: 6 u pi (|sy| + |sx|) -- 4.3e-4 at the largest shift, the
                   dominant term there (the reference's definition shares that rounding; the kernels reproduce it)
           sincos  sqrt(2) * 1e-6, the accuracy csrc/mc_common.h states for mc_sincos
           ramp    the complex multiply and the scale
         and every pixel |got - ref| <= 10 rel rms(ref) (the fp32 oracle's own error has max / rms <= 8 on every
         case of these tables: tests/test_fourier_reference_host.py).
  sums   sum_f rel_f ||ref_f|| + (t + chunks) u sum_f ||ref_f|| (register accumulators, one add per chunk through
         memory); the exposure-weighted sum adds the filter's rounding chain, proportional to 1 + N_f / (2 N_c);
         raw movies add the conditioning roundings (rigid_reference.conditioning_error) in L2.

Measured worst error / bound per kernel family, from one run on an MI355X (L2 / per pixel); the fp32 CPU oracle's
own error over the same bounds on the same inputs is in the last column (host run, L2 / per pixel):

                                                            kernels          fp32 CPU oracle
  row-major shift, columns 256 .. 2048 (general kernel)       0.059 / 0.027    0.062 / 0.031
  row-major shift, 4096 rows (radix 16)                       0.056 / 0.029    0.061 / 0.034
  row-major shift, 4092 / 8184 rows (mixed radix)             0.057 / 0.031    0.062 / 0.029
  row-major shift, rows of 1024 / 8192 columns                0.053 / 0.029    0.058 / 0.030
  row-major shift, rows of 5760 / 11520 columns               0.065 / 0.033    0.068 / 0.035
  row-major shift, N(5, 2^2) input                            0.022 / 0.009    0.023 / 0.010
  fused sums, plain / exposure-weighted / both                0.050 / 0.025    (worst: (3, 256, 5760); one chunk
                                                                               and several, row- and column-major
                                                                               fed give the same figures)
  fused sums, exposure-weighted without ramp                  0.009 / 0.007
  pruned engine, native lines, N(5, 2^2) input                0.022 / 0.009    0.022 / 0.009
  pruned engine, chirp-z rows (+ columns), odd unpacked rows  0.066 / 0.026    0.066 / 0.026
  pruned engine, 2880 columns direct / by chirp-z             0.074 / 0.031    0.074 / 0.031   (chirp-z: 0.069 / 0.029)
  pruned engine, chirp-z M = 5120 ((2, 96, 5000))             0.056 / 0.029    0.056 / 0.028
  mc_dose_accumulate                                          0.010 / 0.005
  polyphase shift, forced / natural 16384 / (2, 96, 7000)     0.053 / 0.025    0.070 / 0.030
  polyphase exposure sum                                      0.021 / 0.015
  raw u8 / i16 (also motion_correct_raw_fast)                 0.042 / 0.021
  fp16 stack                                                  0.016 / 0.007    0.022 / 0.010

At 3 px the kernels' relative L2 error is 4e-7 .. 8e-7, at 40 px 4.9e-6, at 200 px 2.5e-5 -- the figures of torch's
fp32 transform on the CPU -- so mc_sincos meets the accuracy its header states at 1.2e3 rad and no kernel was changed.
Every test of this file takes under a second.
"""

import math

import numpy as np
import pytest
import torch

import fourier_reference as fr
import kernel_harness as kh
from kernel_harness import calls, mc, switches  # noqa: F401
from rigid_reference import condition_float64, conditioning_error

pytestmark = pytest.mark.gpu

U = fr.U


# ------------------------------------------------------------------ comparisons


def _field(shifts, ps=1.0):
    """(2, t, 1, 1) field in Angstrom whose pixel shifts -field / ps are `shifts` (up to the division's rounding:
    the tests read the shifts the kernels get back from the device)."""
    return (-torch.from_numpy(np.asarray(shifts, dtype=np.float32)) * ps).t()[:, :, None, None].contiguous()


def _used_shifts(field_dev, ps):
    """The (t, 2) fp32 shifts the fused routes form from an Angstrom field: engine.fast_shifts(field / ps)."""
    from torch_motion_correction_amd import engine

    return engine.fast_shifts(field_dev / float(ps)).cpu().numpy()


def _assert_frames(got, ref, rel, what):
    """Every frame: finite, relative L2 within rel_f, every pixel within CAP rel_f rms(ref_f).  -> worst ratios."""
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    worst_l2 = worst_px = 0.0
    for f in range(ref.shape[0]):
        l2, mx, _ = fr.measure(got[f], ref[f])
        norm = float(torch.linalg.norm(ref[f]))
        rms = norm / math.sqrt(ref[f].numel())
        print(f"  {what} frame {f}: L2 {l2 / norm:.3e} bound {rel[f]:.3e}; max {mx:.3e} cap {fr.CAP * rel[f] * rms:.3e}")
        assert l2 <= rel[f] * norm, f"{what} frame {f}: relative L2 {l2 / norm:.3e} > {rel[f]:.3e}"
        assert mx <= fr.CAP * rel[f] * rms, f"{what} frame {f}: pixel error {mx:.3e} > {fr.CAP * rel[f] * rms:.3e}"
        worst_l2, worst_px = max(worst_l2, l2 / (rel[f] * norm)), max(worst_px, mx / (fr.CAP * rel[f] * rms))
    return worst_l2, worst_px


def _assert_sum(got, ref, bound, what):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    l2, mx, _ = fr.measure(got, ref)
    cap = fr.CAP * bound / math.sqrt(ref.numel())
    print(f"  {what}: L2 {l2:.3e} bound {bound:.3e}; max {mx:.3e} cap {cap:.3e}")
    assert l2 <= bound, f"{what}: L2 error {l2:.3e} > {bound:.3e}"
    assert mx <= cap, f"{what}: pixel error {mx:.3e} > {cap:.3e}"
    return l2 / bound, mx / cap


class _Worst:
    def __init__(self):
        self.l2 = self.px = 0.0

    def add(self, r):
        self.l2, self.px = max(self.l2, r[0]), max(self.px, r[1])

    def report(self, family):
        print(f"RATIO {family}: L2 {self.l2:.3f} pixel {self.px:.3f}")


def _id(case):
    return "x".join(str(v) for v in case[:3]) + ("-offset" if case[3] is True else "")


def _shift_case(mc, dev, calls, case, layout, family, want, absent=()):
    """correct_motion_fast on every launch of a table case against fourier_shift64; the entry points `want` ran at
    every launch and none of `absent` did."""
    t, h, w, offset = case[:4]
    rel_kinds = None
    worst = _Worst()
    for launch in range(fr.launches(t)):
        x, s, ref = fr.shifted_reference(t, h, w, offset, launch)
        calls.clear()
        got = mc.correct_motion_fast(x.to(dev), _field(s).to(dev))
        torch.cuda.synchronize()
        calls.ran(*want, absent=absent)
        b = fr.bounds(h, w, s, layout)
        rel_kinds = b["kinds"]
        worst.add(_assert_frames(got, ref, b["rel"], f"{family} {case[:3]} shifts {s.tolist()}"))
    worst.report(f"{family} {_id(case)}")
    return rel_kinds


# ------------------------------------------------------------------ the row-major engine: Fourier shift


ROW_MAJOR_ENTRIES = ("mc_full_rows_forward", "mc_full_cols_shift", "mc_full_rows_inverse")
PRUNED_ENTRIES = ("mc_xc_rows_forward", "mc_xcg_rows_forward", "mc_xc_cols_forward", "mc_xcg_cols_forward",
                  "mc_fourier_shift_cols_inverse", "mc_xcg_cols_inverse", "mc_xc_rows_inverse_store",
                  "mc_xcg_rows_inverse", "mc_polyphase_fourier_shift")


@pytest.mark.parametrize("case", fr.ROW_MAJOR_SHIFT, ids=_id)
def test_row_major_fourier_shift(mc, dev, calls, switches, case):
    """mc_full_rows_forward -> mc_full_cols_shift -> mc_full_rows_inverse: the general column kernel at 256 to 2048
    rows, the radix-16 one at 4096, the mixed-radix ones at 4092 / 8184; rows of 64, 1024, 8192, 5760, 11520."""
    engine, _ = switches
    assert engine.FULL_ROW_MAJOR and engine._full_row_major_ok(case[1], case[2])
    _shift_case(mc, dev, calls, case, "row_major", "row-major shift", ROW_MAJOR_ENTRIES, PRUNED_ENTRIES)


# ------------------------------------------------------------------ the row-major engine: fused sums


_REFS = {}


def _sums_reference(key, frames, shifts, expo):
    """shift_sums64, computed once per (case, launch, shifts, exposure)."""
    k = (key, None if shifts is None else shifts.tobytes(), expo)
    if _REFS.get("case") != key[0]:  # one case's references at a time
        _REFS.clear()
        _REFS["case"] = key[0]
    if k not in _REFS:
        ps, dose, pre, kv = expo
        _REFS[k] = fr.shift_sums64(frames, shifts, ps, pre, dose, kv)
    return _REFS[k]


def _cut_workspace(engine, lib, h, w, colmajor):
    """WORKSPACE_BYTES for two frames per chunk of _row_major_sums."""
    per_frame = h * lib.mc_full_spectrum_pitch(w) * 8
    engine.WORKSPACE_BYTES = 2 * (2 if colmajor else 1) * per_frame


_FUSED_PARAMS = [(c, cm, two) for c in fr.FUSED for cm in ((True, False) if c[4] else (True,)) for two in (False, True)]


@pytest.mark.parametrize("case,colmajor,two_per_chunk", _FUSED_PARAMS,
                         ids=[f"{_id(c)}-{'default' if cm else 'row_major_fed'}-{'chunks' if two else 'one'}"
                              for c, cm, two in _FUSED_PARAMS])
def test_fused_shift_sums(mc, dev, calls, switches, case, colmajor, two_per_chunk):
    """mc_full_cols_shift_sum / mc_full_transpose + mc_full_cols_shift_sum_cm in the four modes -- plain (1),
    exposure-weighted (2), both (3), exposure-weighted without ramp (6, dose_weighted_sum) -- in one chunk and with
    two frames per chunk (A and P pass through memory; the last chunk is short for odd t), at the three exposure
    parameter sets."""
    engine, _ = switches
    t, h, w, offset = case[:4]
    assert engine._full_row_major_ok(h, w)
    engine.DOSE_COLUMN_MAJOR = colmajor
    cm = colmajor and h in (4096, 4092)
    if two_per_chunk:
        _cut_workspace(engine, calls._lib, h, w, cm)
    chunks = (t + 1) // 2 if two_per_chunk else 1
    entry, other = ("mc_full_cols_shift_sum_cm", "mc_full_cols_shift_sum") if cm else \
        ("mc_full_cols_shift_sum", "mc_full_cols_shift_sum_cm")
    worst = {m: _Worst() for m in ("plain", "dose", "both", "no ramp")}
    x = fr.case_frames(t, h, w, offset)
    img = x.to(dev)
    for expo in fr.EXPOSURES:
        ps, dose, pre, kv = expo
        expo_term = fr.exposure_term(t, h, w, ps, pre, dose, kv)
        # mode 6: the exposure-weighted sum of the frames as they are
        calls.clear()
        d6 = mc.dose_weighted_sum(img, ps, dose, pre_exposure=pre, voltage=kv)
        torch.cuda.synchronize()
        assert calls.count(entry) == chunks and calls.count(other) == 0 and calls.count("mc_dose_accumulate") == 0
        ref = _sums_reference((case, "still"), x, None, expo)
        rel = fr.bounds(h, w, None, "row_major")["rel"][0] + expo_term + 2 * U
        worst["no ramp"].add(_assert_sum(d6, ref["dw"], fr.sum_l2_bound(rel, ref["norm_d"], chunks),
                                         f"fused {case[:3]} no ramp {expo}"))
        for launch in range(fr.launches(t)):
            s = fr.case_shifts(t)[launch * t:(launch + 1) * t]
            field = _field(s, ps).to(dev)
            used = _used_shifts(field, ps)
            assert np.abs(used - s).max() <= 3 * U * np.abs(s).max()  # the product's and the division's rounding
            ref = _sums_reference((case, launch), x, used, expo)
            b = fr.bounds(h, w, used, "row_major")
            bound_p = fr.sum_l2_bound(b["rel"], ref["norm_y"], chunks)
            bound_d = fr.sum_l2_bound(b["rel"] + expo_term + 2 * U, ref["norm_d"], chunks)
            what = f"fused {case[:3]} {expo} shifts {used.tolist()}"
            calls.clear()
            plain = mc.motion_correct_sum_fast(img, field, ps)
            dw = mc.motion_correct_sum_fast(img, field, ps, dose_per_frame=dose, pre_exposure=pre, voltage=kv)
            dw3, plain3 = mc.motion_correct_sum_fast(img, field, ps, dose_per_frame=dose, pre_exposure=pre, voltage=kv,
                                                     return_plain_sum=True)
            torch.cuda.synchronize()
            assert calls.count(entry) == 3 * chunks and calls.count(other) == 0, (entry, calls.names)
            assert calls.count("mc_full_transpose") == (3 * chunks if cm else 0)
            assert calls.count("mc_full_cols_shift") == 0  # no frame-by-frame composition behind the API
            worst["plain"].add(_assert_sum(plain, ref["plain"], bound_p, what + " [plain]"))
            worst["dose"].add(_assert_sum(dw, ref["dw"], bound_d, what + " [dose]"))
            worst["both"].add(_assert_sum(dw3, ref["dw"], bound_d, what + " [both: dose]"))
            worst["both"].add(_assert_sum(plain3, ref["plain"], bound_p, what + " [both: plain]"))
    for m, wr in worst.items():
        wr.report(f"fused {m} {_id(case)} {'cm' if cm else 'rm'} chunks={chunks}")


# ------------------------------------------------------------------ the pruned engine, transposed layout


_PRUNED_IDS = [f"{_id(c)}-{'direct' if c[4] else 'chirp'}-{c[5]}" for c in fr.PRUNED]


@pytest.mark.parametrize("case", fr.PRUNED, ids=_PRUNED_IDS)
def test_pruned_engine_fourier_shift_and_exposure_sum(mc, dev, calls, switches, case):
    """FULL_ROW_MAJOR off: K1 / K2 forward, then mc_fourier_shift_cols_inverse (native heights) or
    mc_xcg_cols_inverse, and mc_xc_rows_inverse_store (native rows) or mc_xcg_rows_inverse -- native, chirp-z, odd
    unpacked and direct 2880-point lines, the same 2880 columns by chirp-z with USE_DIRECT_LINES off.  The line
    kinds are asserted from the plan, the entry points from the recorder.  dose_weighted_sum (mc_dose_accumulate)
    on the first four shapes."""
    engine, plan = switches
    t, h, w, offset, direct, layout, kinds, with_dose = case
    engine.FULL_ROW_MAJOR = False
    plan.USE_DIRECT_LINES = direct
    plan._LINES.clear()
    got_kinds = fr.transform_cost(h, w, layout)[1]
    assert (got_kinds["rows"], got_kinds["cols"]) == kinds, got_kinds
    plan._LINES.clear()  # the host-side tables above were built for the CPU: the device builds its own
    if layout == "polyphase":
        with pytest.raises(NotImplementedError):
            plan.full_geometry(h, w)
        want = ["mc_polyphase_fourier_shift"]
        hh, ww = h, w // 2
    else:
        want, hh, ww = [], h, w
    g = plan.full_geometry(hh, ww)
    assert plan.native_rows(g) == (kinds[0] == "native") and plan.native_height(hh) == (kinds[1] == "native")
    want += ["mc_xc_rows_forward" if kinds[0] == "native" else "mc_xcg_rows_forward",
             "mc_xc_cols_forward" if kinds[1] == "native" else "mc_xcg_cols_forward",
             "mc_fourier_shift_cols_inverse" if kinds[1] == "native" else "mc_xcg_cols_inverse",
             "mc_xc_rows_inverse_store" if kinds[0] == "native" else "mc_xcg_rows_inverse"]
    absent = [n for n in PRUNED_ENTRIES if n not in want] + list(ROW_MAJOR_ENTRIES)
    _shift_case(mc, dev, calls, case, layout, "pruned shift", want, absent)
    if kinds[1] not in ("native",):
        line, _ = plan.line_plan(hh, +1, dev)
        assert (line.M == hh) == (kinds[1] == "direct"), (line.M, kinds)
    if not with_dose:
        return
    worst = _Worst()
    x = fr.case_frames(t, h, w, offset)
    for expo in fr.EXPOSURES:
        ps, dose, pre, kv = expo
        calls.clear()
        got = mc.dose_weighted_sum(x.to(dev), ps, dose, pre_exposure=pre, voltage=kv)
        torch.cuda.synchronize()
        assert calls.count("mc_dose_accumulate") == 1 and calls.count("mc_full_cols_shift_sum") == 0
        ref = _sums_reference((case, "still"), x, None, expo)
        rel = fr.bounds(h, w, None, layout)["rel"][0] + fr.exposure_term(t, h, w, ps, pre, dose, kv) + 2 * U
        worst.add(_assert_sum(got, ref["dw"], fr.sum_l2_bound(rel, ref["norm_d"]), f"pruned dose {case[:3]} {expo}"))
    worst.report(f"pruned exposure sum {_id(case)}")


# ------------------------------------------------------------------ the x-polyphase form


@pytest.mark.parametrize("case", fr.POLYPHASE, ids=[f"{_id(c)}-{'forced' if c[4] else 'natural'}" for c in fr.POLYPHASE])
def test_polyphase_fourier_shift_and_exposure_sum(mc, dev, calls, switches, case):
    """mc_polyphase_fourier_shift and mc_polyphase_dose_accumulate: forced on frames that do not need it (native
    and chirp-z half frames), and where fourier_shift takes it by itself (16384 columns)."""
    engine, plan = switches
    t, h, w, offset, forced = case
    if forced:
        engine.POLYPHASE_FOURIER_SHIFT = True
    else:
        assert not engine._full_row_major_ok(h, w)
        with pytest.raises(NotImplementedError):
            plan.full_geometry(h, w)
    _shift_case(mc, dev, calls, case, "polyphase", "polyphase shift", ["mc_polyphase_fourier_shift"],
                list(ROW_MAJOR_ENTRIES))
    worst = _Worst()
    x = fr.case_frames(t, h, w, offset)
    for expo in fr.EXPOSURES:
        ps, dose, pre, kv = expo
        calls.clear()
        got = mc.dose_weighted_sum(x.to(dev), ps, dose, pre_exposure=pre, voltage=kv)
        torch.cuda.synchronize()
        assert calls.count("mc_polyphase_dose_accumulate") == 1 and calls.count("mc_dose_accumulate") == 0
        ref = _sums_reference((case, "still"), x, None, expo)
        rel = fr.bounds(h, w, None, "polyphase")["rel"][0] + fr.exposure_term(t, h, w, ps, pre, dose, kv) + 2 * U
        worst.add(_assert_sum(got, ref["dw"], fr.sum_l2_bound(rel, ref["norm_d"]), f"polyphase dose {case[:3]} {expo}"))
    worst.report(f"polyphase exposure sum {_id(case)}")


# ------------------------------------------------------------------ raw bytes


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16], ids=["uint8", "int16"])
@pytest.mark.parametrize("shape", fr.RAW, ids=lambda s: "x".join(str(v) for v in s))
def test_raw_fused_shift_sums(mc, dev, calls, switches, shape, dtype):
    """motion_correct_sum_fast_raw (mc_full_rows_forward_raw) with a gain of large dynamic range: the reference
    conditions in float64 with the kernel's own fp32 means (engine.RawMovie.mu) and the bound carries the
    conditioning roundings, 2 u (|raw gain| + |mu|) per sample, in L2 (a unitary shift and weights <= 1 do not
    amplify them).  (3, 4092, 128): the mixed-radix column pass behind the raw row pass.  The first shape also runs
    motion_correct_raw_fast (estimate + sums from one RawMovie) against the same reference at the field it returns."""
    engine, _ = switches
    t, h, w = shape
    assert engine._full_row_major_ok(h, w)
    raw, gain = kh.raw_movie(t, h, w, dtype, seed=700 + h), kh.gain(h, w)
    rm = engine.RawMovie(raw.to(dev), gain.to(dev))
    mu = rm.mu.cpu().numpy()
    v = condition_float64(raw.numpy(), gain.numpy(), mu)
    cond = float(sum(np.linalg.norm(conditioning_error(raw[f].numpy(), gain.numpy(), mu[f])) for f in range(t)))
    expo = fr.EXPOSURES[1]
    ps, dose, pre, kv = expo
    expo_term = fr.exposure_term(t, h, w, ps, pre, dose, kv)
    worst = _Worst()

    def compare(dw, plain, used, what):
        ref = fr.shift_sums64(v, used, ps, pre, dose, kv)
        b = fr.bounds(h, w, used, "row_major")
        worst.add(_assert_sum(plain, ref["plain"], fr.sum_l2_bound(b["rel"], ref["norm_y"], extra=cond), what + " [plain]"))
        worst.add(_assert_sum(dw, ref["dw"], fr.sum_l2_bound(b["rel"] + expo_term + 2 * U, ref["norm_d"], extra=cond),
                              what + " [dose]"))

    for launch in range(fr.launches(t)):
        s = fr.case_shifts(t)[launch * t:(launch + 1) * t]
        field = _field(s, ps).to(dev)
        used = _used_shifts(field, ps)
        calls.clear()
        dw, plain = mc.motion_correct_sum_fast_raw(raw.to(dev), gain.to(dev), field, ps, dose_per_frame=dose,
                                                   pre_exposure=pre, voltage=kv, return_plain_sum=True)
        torch.cuda.synchronize()
        assert calls.count("mc_full_rows_forward_raw") == 1 and calls.count("mc_full_rows_forward") == 0
        assert calls.count("mc_condition_movie") == 0
        compare(dw, plain, used, f"raw {str(dtype)[6:]} {shape} shifts {used.tolist()}")
    if shape == fr.RAW[0]:
        calls.clear()
        field, dw, plain = mc.motion_correct_raw_fast(raw.to(dev), gain.to(dev), ps, dose_per_frame=dose,
                                                      pre_exposure=pre, voltage=kv, return_plain_sum=True)
        torch.cuda.synchronize()
        assert calls.count("mc_full_rows_forward_raw") == 1 and calls.count("mc_full_rows_forward") == 0
        compare(dw, plain, _used_shifts(field.to(dev), ps), f"motion_correct_raw_fast {str(dtype)[6:]} {shape}")
    worst.report(f"raw {str(dtype)[6:]} {'x'.join(str(n) for n in shape)}")


# ------------------------------------------------------------------ fp16


def test_fp16_stack_fused_shift_sums(mc, dev, calls, switches):
    """An fp16 (3, 512, 512) stack: the same bound on the up-cast values (the widening is exact)."""
    engine, _ = switches
    t, h, w = fr.FP16
    assert engine._full_row_major_ok(h, w)
    half = fr.case_frames(t, h, w, True).half()
    x = half.float()
    expo = fr.EXPOSURES[0]
    ps, dose, pre, kv = expo
    expo_term = fr.exposure_term(t, h, w, ps, pre, dose, kv)
    worst = _Worst()
    for launch in range(fr.launches(t)):
        s = fr.case_shifts(t)[launch * t:(launch + 1) * t]
        field = _field(s, ps).to(dev)
        used = _used_shifts(field, ps)
        calls.clear()
        dw, plain = mc.motion_correct_sum_fast(half.to(dev), field, ps, dose_per_frame=dose, pre_exposure=pre,
                                               voltage=kv, return_plain_sum=True)
        torch.cuda.synchronize()
        assert calls.count("mc_full_cols_shift_sum") == 1
        ref = fr.shift_sums64(x, used, ps, pre, dose, kv)
        b = fr.bounds(h, w, used, "row_major")
        what = f"fp16 {fr.FP16} shifts {used.tolist()}"
        worst.add(_assert_sum(plain, ref["plain"], fr.sum_l2_bound(b["rel"], ref["norm_y"]), what + " [plain]"))
        worst.add(_assert_sum(dw, ref["dw"], fr.sum_l2_bound(b["rel"] + expo_term + 2 * U, ref["norm_d"]), what + " [dose]"))
    worst.report("fp16 3x512x512")
