"""Every kernel of the cross-correlation estimate against the float64 definitions of tests/xc_reference.py, stage by
stage: the forward spectra (workgroup rows + Stockham columns, the wave-per-row K1 of 4096-column frames with row
chords on and off and forced back to the workgroup kernel, radix-16 4096-row and wave 1024-row columns and their
Stockham fallback, the fused-statistics route and its fix-up, fp16 stacks read natively, chirp-z / direct mixed-radix /
odd unpacked lines, patch jobs with per-job mask exponents through the dual wave kernel and through two ordinary
passes, raw u8 / i16 movies and patch jobs), the correlation map seen through its arg-max and 3 x 3 neighbourhood (separate kernels,
the chirp-z engine's, the fused near-window search and its device-side fallback, several workspace chunks), the
parabola on planted fractional drifts, and mc_field_accumulate on hand-built input.  No frame, pair or bin is skipped;
the only tolerance on the arg-max is 2E.  Every test asserts which entry points of libmcorr ran (a recorder around
the loaded library), so a silent fallback cannot pass as coverage.

Bounds (xc_reference's docstring has the derivations; none is fitted to a kernel's output):

  spectra  ||S - S64||_2 <= rel_S ||S64||_2 per job; every kept bin within CAP rel_S filt[bin] rms(unfiltered
           spectrum); filtered-out bins exactly 0.  rel_S = normalisation + mask + forward rows + forward columns
           (pass list of each line's kind, from the plan) + filter; the fused-statistics route adds the fix-up's
           term in |mean - m0| / std and |Mhat[bin]|; raw input adds the conditioning roundings.
  map      E = CAP rel_C rms(cc64), rel_C = both spectra's rel_S + product and scale + inverse columns + rows.
  arg-max  a valid index p with cc64[p] >= max(cc64) - 2E, shifts == wrap(p) exactly.
  nb       |nb - neighbourhood64(cc64, p)| <= E, NaN exactly where the definition has NaN.
  parabola |off - off64| <= E (1 + 4 |off64|) / (|den64| - 4E).
  accumulate  the eight fp32 roundings of a value, counted per entry by accumulate64 (the two inside the parabola's
              denominator amplified by its cancellation): ps ((2 + amp) u |q| + u |f| + u |s|) + u |s ps| + u |field|.

Measured worst error / bound per kernel family, from one run on an MI355X; the fp32 CPU oracle's own ratio over the
same bounds (tests/test_xc_reference_host.py, host run) is in the last column.  Spectra: L2 / per bin; map stages:
arg-max deficit / neighbourhood / parabola (the oracle column adds the map itself, L2 / value, first).

                                                                  kernels          fp32 CPU oracle
  workgroup rows + Stockham columns, 64 .. 512, ps 0.83 / 2.5      0.081 / 0.091    0.078 / 0.090
  wave-per-row K1, (512 | 1024, 4096), bands 10 / 20, chords +/-   0.043 / 0.040    0.041 / 0.037
  the same input forced to the workgroup row kernel                0.046 / 0.039
  radix-16 4096-row columns (Stockham forced: 0.054 / 0.070)       0.052 / 0.069    0.048 / 0.068
  wave 1024-row columns (Stockham forced: 0.030 / 0.017)           0.028 / 0.017    0.022 / 0.017
  benchmark geometry (3, 4096, 4096), fused statistics             0.016 / 0.012    0.014 / 0.007
  wide band, nkx > 512 on 4096 columns                             0.025 / 0.036    0.024 / 0.035
  fused statistics N(0, 1) / N(40, 2.5^2) / N(1000, 30^2)          0.023 / 0.013    0.018 / 0.009 (N(1000, 30^2): 0.418 / 0.414)
  fp16 stack (2, 4096, 4096), read natively through the engine     0.017 / 0.009
  fp16 stack (2, 1024, 4096), widened once by the engine           0.020 / 0.020
  chirp-z rows and columns, output-pruned and odd unpacked rows    0.027 / 0.012    0.027 / 0.012
  direct 2880-point lines (by chirp-z: 0.020 / 0.014)              0.048 / 0.036    0.048 / 0.037
  chirp-z M = 5120, 10240, 16384                                   0.016 / 0.009    0.013 / 0.009
  patch jobs 1024, dual wave kernel, fp32 / fp16                   0.025 / 0.035    0.023 / 0.031
  patch jobs 1024 / 48 / 63 / 80, two ordinary passes              0.033 / 0.030    0.031 / 0.008
  raw patch jobs 1024, u8 / i16 + gain, dual / single              0.020 / 0.014    0.016 / 0.006
  raw patch jobs (16, 1024): ny = 16, the group tail (1024: 800)   0.026 / 0.007    0.035 / 0.005
  raw u8 / i16, gain 1 +- 0.05, 1024 / 4096 / 5760 / 11520 columns 0.035 / 0.013
  the same movies, gain log-uniform in [0.25, 4]                   0.027 / 0.013
  raw (2, 512, 4096) without row chords, both gains                0.020 / 0.012
  separate kernels 256 / 512: arg-max / nb / parabola              0 / 0.079 / 0.017      0.012 / 0.058; 0 / 0.058 / 0.007
  chirp-z engine (mc_xcg_*) (100, 120), (121, 135), (96, 5760)     0 / 0.033 / 0.004      0.005 / 0.020; 0 / 0.020 / 0.003
  fused near-window search (1024, 1024), (4096, 256)               0 / 0.159 / 0.040      0.013 / 0.093; 0 / 0.092 / 0.019
  the same pairs with FUSED_SEARCH = False                         0 / 0.207 / 0.040
  parabola on planted fractional drifts                            0.018
  mc_field_accumulate (flags 0 .. 3)                               0.626

The N(1000, 30^2) row shows why the route subtracts a provisional mean: the oracle, which subtracts the fp32 mean
from fp32 counts, uses 0.42 of the bound's (5 + |mean| / std) u normalisation term; the kernels stay at 0.02.  Every
arg-max is the unique float64 maximum on the planted cases and admissible on the noise and near-tie cases (deficit 0
in all).  The near-tie cases ('tie': xc_reference.tied, two exactly tied maxima at +s and -s) are the ones that take the
tolerant branch of the criterion, on the separate, the chirp-z and the fused path; white noise almost never ties
within 2E, so the pure-noise cases mostly reduce to the unique maximum and are kept as the inputs on which the
branch and bound cannot prune.  mc_xcg_peak_neighbourhood is judged against E alone, like the row transform.  No
kernel is outside its bound and none was changed.

The raw patch jobs (mc_xc_rows_forward_dual_raw: the wave-per-patch-row kernel reading u8 / i16 bytes and the gain)
run on xc_reference.raw_patch_input: frames of an odd width, jobs at odd origins in both frames and not sorted by
frame, a gain of dynamic range 16, a brighter second frame (so the per-job subtrahends differ), i16 counts negative
in both halves of a pair, the (1, 2) exponent pair and the power loops in one launch; dual and single, row chords
on and off, in workspace chunks, and on the one plan whose ny % 32 != 0 (window (16, 1024): ny = 16; (1024, 1024):
ny = 800).  tests/test_xc_reference_host.py holds an fp32 restatement of that pass on the same input inside the same
bounds (the oracle column) and plants the faults the RAW branch could make, each of which leaves the bound.

On the MI355X the file's 138 tests take 16 s in all; the (3, 4096, 4096) case is the slowest with 2.0 s, the first
raw patch test, which builds the float64 reference the others share, takes 1.1 s, every other test stays under 0.8 s.
"""

import contextlib
import math

import numpy as np
import pytest
import torch

import xc_reference as xr
from global_refine_reference import planted_movie
import kernel_harness
from kernel_harness import calls, nan_empty, switches  # noqa: F401
from rigid_reference import condition_float64, conditioning_error

pytestmark = pytest.mark.gpu

U = xr.U
MC_STORE_U8, MC_STORE_I16, STORE_F16, STORE_F32 = 0, 1, 2, 3  # MC_STORE_* of include/mcorr.h


@contextlib.contextmanager
def engines(row=0, col=0):
    """mc_xc_row_engine / mc_xc_col_engine forced for the block, both back to automatic afterwards."""
    from torch_motion_correction_amd import _lib

    lib = _lib.load()
    try:
        assert lib.mc_xc_row_engine(row) == 0 and lib.mc_xc_col_engine(col) == 0
        yield
    finally:
        lib.mc_xc_row_engine(0)
        lib.mc_xc_col_engine(0)


def _plan(pa, dev):
    from torch_motion_correction_amd import plan

    h, w, ps, b, band = pa
    return plan.get_xc_plan(h, w, ps, b, band, dev)


def _stats_tensor(mean, std, dev):
    return torch.tensor([mean, 1.0 / std, std], dtype=torch.float32, device=dev)


def _frame_offsets(t, h, w, dev):
    return torch.arange(t, device=dev, dtype=torch.int64) * (h * w)


def _fused_terms(x, pa, parts):
    """(d, Mhat64) of the fused-statistics route: m0 is the mean of the first box row of frame 0
    (engine._global_spectra)."""
    h, w = pa[:2]
    hl, wl, wu = int(0.25 * h), int(0.25 * w), int(0.75 * w)
    m0 = float(x[0, hl, wl:wu].double().mean())
    return abs(parts["mean"] - m0) / parts["std"], xr.mask_spectrum64(pa)


def _fused_terms_box(x, box, mean, std, pa):
    hl, _, wl, wu = box
    m0 = float(x[0, hl, wl:wu].double().mean())
    return abs(mean - m0) / std, xr.mask_spectrum64(pa)


def _box_stats(x, box):
    hl, hu, wl, wu = box
    b = x[:, hl:hu, wl:wu].double()
    return float(b.mean()), float(b.std())


def _fused_route(engine, img, pl, box):
    """The fused-statistics route of engine._global_spectra, launch for launch, with the statistics box given -- for
    the one case the engine cannot be steered to: a box OFF the 256-sample chunk grid on 4096-column rows, where the
    statistics stay on the workgroup form of mc_xc_rows_forward_stats_t (every box the engine forms on such rows is on
    the grid).  Everything else goes through the engine's own seams."""
    import ctypes as C

    from torch_motion_correction_amd import _lib
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    lib = _lib.load()
    t, h, w = img.shape
    dev, g = img.device, pl.geom
    hl, hu, wl, wu = box
    assert g.y0 <= hl and hu <= g.y0 + g.ny and g.x0 <= wl and wu <= g.x1 and wl % 2 == 0 and wu % 2 == 0
    st = stream_ptr(dev)
    mhat = engine.mask_spectrum(pl, dev)
    off = _frame_offsets(t, h, w, dev)
    acc = torch.empty(128, dtype=torch.float64, device=dev)
    m0 = torch.empty(3, dtype=torch.float32, device=dev)
    check(lib.mc_xc_provisional_mean_t(C.c_void_p(img.data_ptr() + img.element_size() * (hl * w + wl)),
                                       engine.storage_of(img), wu - wl, ptr(m0), st), "mc_xc_provisional_mean_t")
    fix = torch.empty(2, dtype=torch.float32, device=dev)
    out3 = torch.empty(3, dtype=torch.float32, device=dev)
    T1 = torch.empty((t, g.nkx, g.ny, 2), dtype=torch.float32, device=dev)
    S = torch.empty((t, g.nkx, g.nky, 2), dtype=torch.float32, device=dev)
    check(lib.mc_xc_rows_forward_stats_t(ptr(img), engine.storage_of(img), ptr(off), w, ptr(pl.mask), ptr(m0), ptr(T1),
                                         ptr(pl.tw_row), t, g, hl, hu, wl, wu, ptr(acc), ptr(fix), ptr(out3),
                                         ptr(engine._box_chords(pl, hl, hu, wl, wu)), st), "mc_xc_rows_forward_stats_t")
    check(lib.mc_xc_cols_forward_fix(ptr(T1), ptr(pl.filt), ptr(S), ptr(pl.tw_col), t, g, ptr(fix), ptr(mhat), st),
          "mc_xc_cols_forward_fix")
    torch.cuda.synchronize()
    return S, out3.cpu().numpy()


def _plain_spectra(engine, x, pa, parts, pl, dev):
    """The kernels' spectra by the plain row and column passes with the float64 statistics (rounded to fp32)."""
    t, h, w = x.shape
    return engine._forward_spectra(x.to(dev), _frame_offsets(t, h, w, dev), w, None, pl,
                                   _stats_tensor(parts["mean"], parts["std"], dev))


def _rows_entry(plan, g):
    return "mc_xc_rows_forward" if plan.native_rows(g) else "mc_xcg_rows_forward"


def _cols_entry(plan, g):
    return "mc_xc_cols_forward" if plan.native_height(g.H) else "mc_xcg_cols_forward"


def _both_seams(engine, plan, calls, dev, x, pa, what, expect_fused):
    """One stack through engine._forward_spectra with supplied statistics (the plain row and column passes) and
    through engine._global_spectra (statistics inside; the fused-statistics route exactly where `expect_fused` says the
    engine takes it), each against spectra64 with its own bound.  -> worst (L2, bin) ratios."""
    t, h, w = x.shape
    pl = _plan(pa, dev)
    g = pl.geom
    parts = xr.spectra_parts(x, pa)
    plain = xr.spectra_bounds(pa, parts["mean"], parts["std"])
    xd = x.to(dev)
    calls.clear()
    S = engine._forward_spectra(xd, _frame_offsets(t, h, w, dev), w, None, pl,
                                _stats_tensor(parts["mean"], parts["std"], dev))
    torch.cuda.synchronize()
    calls.ran(_rows_entry(plan, g), _cols_entry(plan, g), absent=("mc_xc_rows_forward_stats_t", "mc_xc_cols_forward_fix"))
    r1 = xr.check_spectra(S, parts, plain, f"{what} rows+cols")
    calls.clear()
    S = engine._global_spectra(xd, pl)
    torch.cuda.synchronize()
    fused = calls.count("mc_xc_rows_forward_stats_t") >= 1
    assert fused == expect_fused, f"{what}: fused statistics {fused}, expected {expect_fused}"
    if fused:
        calls.ran("mc_xc_provisional_mean_t", "mc_xc_cols_forward_fix", absent=("mc_central_box_stats_t",))
        b = xr.spectra_bounds(pa, parts["mean"], parts["std"], fused=_fused_terms(x, pa, parts))
    else:
        calls.ran("mc_central_box_stats_t", _rows_entry(plan, g), _cols_entry(plan, g))
        b = plain
    r2 = xr.check_spectra(S, parts, b, f"{what} global{' fused' if fused else ''}")
    print(f"RATIO {what} {b['kinds']}: rows+cols L2 {r1[0]:.3f} bin {r1[1]:.3f}; global{' fused' if fused else ''} "
          f"L2 {r2[0]:.3f} bin {r2[1]:.3f}")
    return r1, r2


def _case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}-{c[3]:g}-{c[4][1]:g}"


# ------------------------------------------------------------------ forward spectra


@pytest.mark.parametrize("case", xr.SPECTRA_SMALL, ids=_case_id)
def test_workgroup_rows_stockham_columns_and_chirp_z_lines(dev, calls, switches, case):
    """Power-of-two frames of 64 .. 512 on the workgroup row kernel and the Stockham columns (pixel spacings 0.83 and
    2.5: the wide band keeps more bins), and the chirp-z engine: both axes, output-pruned rows of 1440 columns, odd
    unpacked rows of 135."""
    engine, plan = switches
    t, h, w, ps, band = case
    _both_seams(engine, plan, calls, dev, xr.noise(t, h, w, mean=5.0, std=2.0), xr.args(h, w, ps, band), f"small {case[:3]}",
                expect_fused=(h == w and plan.native_width(w)))  # near-square native frames: the box lies inside what K1 reads


LINE_CASES = [(c, True) for c in xr.SPECTRA_LINES] + [(c, False) for c in xr.SPECTRA_LINES if c[2] == 5760 or c[1] == 2880]


@pytest.mark.parametrize("case,direct", LINE_CASES, ids=lambda v: _case_id(v) if isinstance(v, tuple) else f"direct={v}")
def test_direct_mixed_radix_and_long_chirp_z_lines(dev, calls, switches, case, direct):
    """Rows of 5760 columns and columns of 2880 rows transformed directly and (USE_DIRECT_LINES = False) by chirp-z;
    rows of 7000 columns (forward M = 5120), columns of 4100 rows (M = 10240) and of 5200 rows (M = 16384)."""
    engine, plan = switches
    t, h, w, ps, band = case
    plan.USE_DIRECT_LINES = direct
    pa = xr.args(h, w, ps, band)
    kinds = xr.line_costs(xr.geometry(pa))["kinds"]
    assert ("direct" in kinds.values()) == (direct and (w == 5760 or h == 2880)), kinds
    _both_seams(engine, plan, calls, dev, xr.noise(t, h, w, mean=5.0, std=2.0), pa, f"lines {case[:3]} direct={direct}",
                expect_fused=False)


@pytest.mark.parametrize("chords", [True, False])
@pytest.mark.parametrize("row_engine", [0, 1])
@pytest.mark.parametrize("case", xr.SPECTRA_WIDE[:4], ids=_case_id)
def test_wave_per_row_k1(dev, calls, switches, case, row_engine, chords):
    """Rows of 4096 columns: one wavefront per row (row engine 0) and the workgroup kernel forced on the same input
    (row engine 1), row chords on and off, bands (300, 10) and (300, 20) (nkx <= 256); h = 512 puts the mask support
    inside two chunks of the row (clamped loads) and its statistics box off the chunk grid, h = 1024 is fused-eligible
    on the wave kernel (test_fused_statistics_and_fix_up; here the plain row pass mc_xc_rows_forward, which the
    engine takes for these frames because their default box lies outside the columns K1 reads)."""
    engine, plan = switches
    t, h, w, ps, band = case
    engine.USE_ROW_CHORDS = chords
    pa = xr.args(h, w, ps, band)
    assert (xr.geometry(pa).nkx <= 256) == (band[1] == 20.0)
    with engines(row=row_engine):
        _both_seams(engine, plan, calls, dev, xr.noise(t, h, w, mean=5.0, std=2.0), pa,
                    f"K1 {case[:3]} band {band[1]:g} engine {row_engine} chords {chords}", expect_fused=False)


@pytest.mark.parametrize("col_engine", [0, 1])
@pytest.mark.parametrize("case", xr.SPECTRA_WIDE[4:], ids=_case_id)
def test_radix16_and_wave_columns(dev, calls, switches, case, col_engine):
    """Columns of 4096 rows (register-resident radix 16) and of 1024 rows (one wavefront per column), and both
    forced to the Stockham passes."""
    engine, plan = switches
    t, h, w, ps, band = case
    with engines(col=col_engine):
        _both_seams(engine, plan, calls, dev, xr.noise(t, h, w, mean=5.0, std=2.0), xr.args(h, w, ps, band),
                    f"columns {case[:3]} engine {col_engine}", expect_fused=False)


def test_wide_band_keeps_more_than_512_columns(dev, calls, switches):
    """A band to 3 A on 4096-column frames keeps nkx > 512 columns: outside what the wave-per-row K1 takes (the recorder
    sees the shared entry point mc_xc_rows_forward; the bound is what tells a wrong kernel)."""
    engine, plan = switches
    t, h, w, ps, band = xr.WIDE_BAND
    pa = xr.args(h, w, ps, band)
    assert xr.geometry(pa).nkx > 512
    _both_seams(engine, plan, calls, dev, xr.noise(t, h, w, mean=5.0, std=2.0), pa, f"wide band {xr.WIDE_BAND[:3]}",
                expect_fused=False)


def test_benchmark_geometry(dev, calls, switches):
    """(3, 4096, 4096) through engine._global_spectra: the benchmark's K1 + K2 with the fused statistics."""
    engine, plan = switches
    t, h, w, ps, band = xr.BENCH
    pa = xr.args(h, w, ps, band)
    x = xr.noise(t, h, w, mean=5.0, std=2.0)
    parts = xr.spectra_parts(x, pa)
    pl = _plan(pa, dev)
    engine.mask_spectrum(pl, dev)  # built once per plan by the plain passes: before the recorder starts
    calls.clear()
    S = engine._global_spectra(x.to(dev), pl)
    torch.cuda.synchronize()
    calls.ran("mc_xc_rows_forward_stats_t", "mc_xc_cols_forward_fix", absent=("mc_central_box_stats_t", "mc_xc_rows_forward"))
    b = xr.spectra_bounds(pa, parts["mean"], parts["std"], fused=_fused_terms(x, pa, parts))
    r = xr.check_spectra(S, parts, b, "benchmark geometry")
    print(f"RATIO benchmark geometry (3, 4096, 4096) fused: L2 {r[0]:.3f} bin {r[1]:.3f} (d = {b['d']:.3f})")


FUSED_BOXES = {(1, 4096, 4096): None,                    # the engine's own route; box on the 256-sample chunk grid: wave kernel
               (2, 512, 4096): (128, 384, 1900, 2200),   # off the chunk grid: the statistics stay on the workgroup kernel
               (2, 256, 256): None}                      # the engine's own route, workgroup kernel throughout


@pytest.mark.parametrize("shape", list(FUSED_BOXES), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mean,std", xr.STAT_INPUTS)
def test_fused_statistics_and_fix_up(dev, calls, switches, shape, mean, std):
    """mc_xc_rows_forward_stats_t + mc_xc_cols_forward_fix on N(0, 1), N(40, 2.5^2) and counts-like N(1000, 30^2): the
    provisional mean keeps d = |mean - m0| / std small, so the fix-up's term stays small and the bound barely moves --
    a route that subtracted nothing would need d = 33 on the last input.  The statistics the kernel returns are
    within their roundings of the float64 ones."""
    engine, plan = switches
    t, h, w = shape
    pa = xr.args(h, w)
    x = xr.noise(t, h, w, mean=mean, std=std)
    pl = _plan(pa, dev)
    box = FUSED_BOXES[shape]
    engine.mask_spectrum(pl, dev)  # built once per plan by the plain passes: before the recorder starts
    calls.clear()
    if box is None:
        S = engine._global_spectra(x.to(dev), pl)
        torch.cuda.synchronize()
        box = (int(0.25 * h), int(0.75 * h), int(0.25 * w), int(0.75 * w))
    else:
        S, out3 = _fused_route(engine, x.to(dev), pl, box)
        m64, s64 = _box_stats(x, box)
        assert abs(out3[0] - m64) <= 2 * U * abs(m64) + 1e-7 * s64 and abs(out3[2] - s64) <= 8 * U * s64 * (1 + abs(m64) / s64)
    calls.ran("mc_xc_provisional_mean_t", "mc_xc_rows_forward_stats_t", "mc_xc_cols_forward_fix",
              absent=("mc_central_box_stats_t", "mc_xc_rows_forward", "mc_xc_cols_forward"))
    m64, s64 = _box_stats(x, box)
    parts = xr.spectra_parts(x, pa, stats=(m64, s64))
    d, mhat = _fused_terms_box(x, box, m64, s64, pa)
    assert d < 0.5, f"the provisional mean is {d:.2f} std from the mean"
    b = xr.spectra_bounds(pa, m64, s64, fused=(d, mhat))
    r = xr.check_spectra(S, parts, b, f"fused statistics {shape} N({mean:g}, {std:g}^2)")
    print(f"RATIO fused statistics {shape} N({mean:g}, {std:g}^2) d={d:.3f}: L2 {r[0]:.3f} bin {r[1]:.3f}")


def test_fp16_stack_is_read_natively(dev, calls, switches):
    """An fp16 (2, 4096, 4096) stack through engine._global_spectra: the engine decides (half_ok) to hand the fp16
    tensor itself to the wave-per-row K1 -- the recorder sees the caller's data pointer with MC_STORE_F16 in the
    provisional mean and in the ONE call of mc_xc_rows_forward_stats_t (a refused first attempt would show as a
    second call with a widened copy) -- and the results are those of the exact up-cast, so the bound is the fp32
    one."""
    engine, plan = switches
    t, h, w = 2, 4096, 4096
    pa = xr.args(h, w)
    x16 = xr.noise(t, h, w, mean=5.0, std=2.0).half()
    pl = _plan(pa, dev)
    engine.mask_spectrum(pl, dev)
    xd = x16.to(dev)
    calls.clear()
    S = engine._global_spectra(xd, pl)
    torch.cuda.synchronize()
    calls.ran("mc_xc_rows_forward_stats_t", "mc_xc_cols_forward_fix", absent=("mc_central_box_stats_t", "mc_xc_rows_forward"))
    a = calls.args["mc_xc_rows_forward_stats_t"]
    assert len(a) == 1 and a[0][1] == STORE_F16 and a[0][0].value == xd.data_ptr(), "the fp16 stack was widened"
    assert calls.args["mc_xc_provisional_mean_t"][0][1] == STORE_F16
    parts = xr.spectra_parts(x16, pa)
    b = xr.spectra_bounds(pa, parts["mean"], parts["std"], fused=_fused_terms(x16, pa, parts))
    r = xr.check_spectra(S, parts, b, "fp16 stack")
    print(f"RATIO fp16 stack (2, 4096, 4096): L2 {r[0]:.3f} bin {r[1]:.3f}")


def test_fp16_stack_of_wide_frames_is_widened_once(dev, calls, switches):
    """(2, 1024, 4096) fp16 was meant to be read natively; frames of 4096 columns that are not near-square never take
    the fused-statistics route (their default box lies outside the columns K1 reads), and only that route reads
    fp16: the engine widens the stack once and takes the separate statistics pass and the plain row pass on fp32 --
    asserted as what it is, against the float64 spectra of the fp16 values."""
    engine, plan = switches
    t, h, w = 2, 1024, 4096
    pa = xr.args(h, w)
    x16 = xr.noise(t, h, w, mean=5.0, std=2.0).half()
    pl = _plan(pa, dev)
    xd = x16.to(dev)
    calls.clear()
    S = engine._global_spectra(xd, pl)
    torch.cuda.synchronize()
    calls.ran("mc_central_box_stats_t", "mc_xc_rows_forward", "mc_xc_cols_forward", absent=("mc_xc_rows_forward_stats_t",))
    assert calls.args["mc_central_box_stats_t"][0][1] == STORE_F32 and calls.args["mc_xc_rows_forward"][0][0].value != xd.data_ptr()
    parts = xr.spectra_parts(x16, pa)
    r = xr.check_spectra(S, parts, xr.spectra_bounds(pa, parts["mean"], parts["std"]), "fp16 wide frames, widened")
    print(f"RATIO fp16 stack (2, 1024, 4096), widened by the engine: L2 {r[0]:.3f} bin {r[1]:.3f}")


# ------------------------------------------------------------------ patch jobs


PATCH_JOBS = [(0, 1, 3), (1, 7, 13), (0, 9, 5), (1, 0, 1)]  # (frame, y0, x0): origins that are no multiple of 4 samples


def _patch_input(p, dev, half=False):
    H, W = p + 9, p + 14
    x = xr.noise(2, H, W, mean=5.0, std=2.0)
    x = x.half() if half else x
    off = torch.tensor([f * H * W + y0 * W + x0 for f, y0, x0 in PATCH_JOBS], dtype=torch.int64, device=dev)
    assert sum(int(o) % 4 != 0 for o in off) >= 2
    return x, off, W


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_patch_jobs_dual_wave_kernel(dev, calls, switches, half):
    """1024-px patches, per-job exponents (1, 2, 3, 1) and their doubles from ONE read of the rows
    (mc_xc_rows_forward_dual_t), fp32 and fp16 (read natively)."""
    engine, plan = switches
    p = 1024
    pa = xr.args(p, p)
    x, off, W = _patch_input(p, dev, half)
    ea, eb = [1, 2, 3, 1], [2, 4, 6, 2]
    mean, std = xr.box_stats64(x)
    pl = _plan(pa, dev)
    calls.clear()
    Sa, Sb = engine._forward_spectra(x.to(dev), off, W, torch.tensor(ea, dtype=torch.int32, device=dev), pl,
                                     _stats_tensor(mean, std, dev),
                                     job_expo_b=torch.tensor(eb, dtype=torch.int32, device=dev), min_expo=1)
    torch.cuda.synchronize()
    calls.ran("mc_xc_rows_forward_dual_t", "mc_xc_cols_forward", absent=("mc_xc_rows_forward",))
    assert calls.args["mc_xc_rows_forward_dual_t"][0][1] == (STORE_F16 if half else STORE_F32)
    for S, ex, tag in ((Sa, ea, "a"), (Sb, eb, "b")):
        parts = xr.spectra_parts(x, pa, PATCH_JOBS, ex, (mean, std))
        r = xr.check_spectra(S, parts, [xr.spectra_bounds(pa, mean, std, expo=e) for e in ex], f"dual {tag} half={half}")
        print(f"RATIO patch jobs 1024 dual wave kernel {'fp16' if half else 'fp32'} {tag}: L2 {r[0]:.3f} bin {r[1]:.3f}")


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
def test_patch_jobs_single_wave_kernel(dev, calls, switches, half):
    """The same 1024-px jobs with ONE exponent per job (the middle-frame strategy's call of
    mc_xc_rows_forward_dual_t: no second exponent list, no second T1), fp32 and fp16: the single-spectrum form of
    the wave-per-patch-row kernel, against the bounds of the dual form's first spectrum."""
    engine, plan = switches
    p = 1024
    pa = xr.args(p, p)
    x, off, W = _patch_input(p, dev, half)
    ea = [1, 2, 3, 1]
    mean, std = xr.box_stats64(x)
    pl = _plan(pa, dev)
    calls.clear()
    S = engine._forward_spectra(x.to(dev), off, W, torch.tensor(ea, dtype=torch.int32, device=dev), pl,
                                _stats_tensor(mean, std, dev), min_expo=1)
    torch.cuda.synchronize()
    calls.ran("mc_xc_rows_forward_dual_t", "mc_xc_cols_forward", absent=("mc_xc_rows_forward",))
    a = calls.args["mc_xc_rows_forward_dual_t"]
    assert len(a) == 1 and a[0][1] == (STORE_F16 if half else STORE_F32) and a[0][5] is None and a[0][9] is None
    parts = xr.spectra_parts(x, pa, PATCH_JOBS, ea, (mean, std))
    r = xr.check_spectra(S, parts, [xr.spectra_bounds(pa, mean, std, expo=e) for e in ea], f"single half={half}")
    print(f"RATIO patch jobs 1024 single wave kernel {'fp16' if half else 'fp32'}: L2 {r[0]:.3f} bin {r[1]:.3f}")


@pytest.mark.parametrize("p", [1024, 48, 63, 80])
def test_patch_jobs_two_ordinary_passes(dev, calls, switches, p):
    """The same jobs where the engine has no fused kernel (no host-known minimum exponent for 1024, any other patch
    size): two ordinary passes with per-job exponents -- the workgroup kernel for 1024, chirp-z rows and columns for
    48, 63 (odd, unpacked) and 80."""
    engine, plan = switches
    pa = xr.args(p, p)
    x, off, W = _patch_input(p, dev)
    ea, eb = [1, 2, 3, 1], [2, 4, 6, 2]
    mean, std = xr.box_stats64(x)
    pl = _plan(pa, dev)
    calls.clear()
    Sa, Sb = engine._forward_spectra(x.to(dev), off, W, torch.tensor(ea, dtype=torch.int32, device=dev), pl,
                                     _stats_tensor(mean, std, dev),
                                     job_expo_b=torch.tensor(eb, dtype=torch.int32, device=dev), min_expo=None)
    torch.cuda.synchronize()
    calls.ran(_rows_entry(plan, pl.geom), _cols_entry(plan, pl.geom), absent=("mc_xc_rows_forward_dual_t",))
    assert calls.count(_rows_entry(plan, pl.geom)) == 2
    for S, ex, tag in ((Sa, ea, "a"), (Sb, eb, "b")):
        parts = xr.spectra_parts(x, pa, PATCH_JOBS, ex, (mean, std))
        r = xr.check_spectra(S, parts, [xr.spectra_bounds(pa, mean, std, expo=e) for e in ex], f"patches {p} {tag}")
        print(f"RATIO patch jobs {p} two passes {tag}: L2 {r[0]:.3f} bin {r[1]:.3f}")


# ------------------------------------------------------------------ raw patch jobs


def _arg(name, param):
    """Position of the argument `param` of the entry point `name`, read from its declaration in include/mcorr.h (and
    the declaration has as many arguments as _lib.SIGNATURES[name])."""
    import re

    from torch_motion_correction_amd import _lib

    names = [re.search(r"(\w+)\s*$", a).group(1) for a in kernel_harness.header_parameters(name)]
    assert len(names) == len(_lib.SIGNATURES[name]) and names.count(param) == 1, (name, names)
    return names.index(param)


@pytest.fixture
def nan_outputs(monkeypatch, nan_empty):  # noqa: F811
    """kernel_harness.nan_empty, and the same for torch.empty_like: the dual form's second spectrum and second T1 are
    allocated with it, and a buffer the allocator hands out again may hold the previous test's correct values."""
    real = torch.empty_like

    def empty_like(*a, **k):
        out = real(*a, **k)
        return out.fill_(float("nan")) if out.is_floating_point() else out

    monkeypatch.setattr(torch, "empty_like", empty_like)


def _raw_patch_spectra(engine, calls, dev, kind, h, dual):
    """xr.RAW_PATCH_JOBS of xr.raw_patch_input(kind, h) through the engine's own seam, engine.raw._patch_spectra_raw
    -> (sub, rstd read back from the RawMovie, plan args, S or (Sa, Sb)); the recorder holds that call alone."""
    raw, gain = xr.raw_patch_input(kind, h)
    _, H, W = raw.shape
    rm = engine.RawMovie(raw.to(dev), gain.to(dev))
    pa = xr.args(h, 1024)
    pl = _plan(pa, dev)
    off = torch.tensor(xr.check_raw_patch_jobs(h), dtype=torch.int64, device=dev)
    ea, eb = (torch.tensor(e, dtype=torch.int32, device=dev) for e in xr.RAW_PATCH_EXPO)
    frames = np.array([f for f, _, _ in xr.RAW_PATCH_JOBS])
    calls.clear()
    out = engine.raw._patch_spectra_raw(rm, pl)(off, ea, frames, eb if dual else None, min_expo=1)
    torch.cuda.synchronize()
    calls.ran("mc_xc_rows_forward_dual_raw", "mc_xc_cols_forward",
              absent=("mc_xc_rows_forward", "mc_xc_rows_forward_dual_t", "mc_condition_movie"))
    name = "mc_xc_rows_forward_dual_raw"
    for a in calls.args[name]:
        assert a[_arg(name, "storage")] == {"u8": MC_STORE_U8, "i16": MC_STORE_I16}[kind]
        assert a[_arg(name, "frame_area")] == H * W and a[_arg(name, "row_stride")] == W
        assert (a[_arg(name, "expo_b")] is not None) == dual and (a[_arg(name, "T1b")] is not None) == dual
        assert (a[_arg(name, "row_chord")] is not None) == bool(engine.USE_ROW_CHORDS)
    sub, rstd = rm.sub.cpu().numpy(), float(rm.mean_rstd.cpu()[1])
    # a job that took the other frame's subtrahend would be off by a constant of this many standard deviations
    assert float(sub[1] - sub[0]) >= 0.25 * abs(float(sub[0])) and float(sub[1] - sub[0]) * rstd >= 0.25, (sub, rstd)
    return sub, rstd, pa, out


def _raw_patch_check(kind, pa, sub, rstd, spectra, what):
    worst = []
    for S, ex, tag in zip(spectra, xr.RAW_PATCH_EXPO, "ab"):
        parts, bounds = xr.raw_patch_reference(kind, pa, sub, rstd, ex)
        r = xr.check_spectra(S, parts, bounds, f"{what} {tag}")
        print(f"RATIO raw patch jobs {what} {tag} (conditioning {bounds[0]['conditioning'] / U:.1f} u of "
              f"{bounds[0]['rel'] / U:.0f} u): L2 {r[0]:.3f} bin {r[1]:.3f}")
        worst.append(r)
    return worst


@pytest.mark.parametrize("chords", [True, False], ids=["chords", "no-chords"])
@pytest.mark.parametrize("kind", ["u8", "i16"])
def test_raw_patch_jobs_dual(dev, calls, switches, nan_outputs, kind, chords):
    """mc_xc_rows_forward_dual_raw, both spectra from one read of the raw rows: five 1024-px jobs in two frames of
    (1033, 1039) u8 / i16 counts -- an odd frame width, which engine.RawMovie and mc_raw_movie_stats take (the scalar
    statistics kernel) -- not sorted by frame, at odd origins, one at the origin of frame 1; a gain of dynamic range
    16; frame 1 brighter, so the per-job subtrahends differ; i16 counts negative in both halves of a pair; exponents
    (1, 2, 3, 1, 1) and (2, 4, 6, 2, 2): the (1, 2) fast path and the power loops in one launch; row chords on and
    off.  Against the float64 conditioning with the statistics the kernel was given, output buffers NaN-filled."""
    engine, plan = switches
    engine.USE_ROW_CHORDS = chords
    sub, rstd, pa, out = _raw_patch_spectra(engine, calls, dev, kind, 1024, dual=True)
    assert calls.count("mc_xc_rows_forward_dual_raw") == 1 and calls.count("mc_xc_cols_forward") == 2
    _raw_patch_check(kind, pa, sub, rstd, out, f"1024 {kind} dual chords={chords}")


@pytest.mark.parametrize("kind", ["u8", "i16"])
def test_raw_patch_jobs_single(dev, calls, switches, nan_outputs, kind):
    """The same jobs with one exponent per job (no second exponent list, no second T1): the single-spectrum form,
    whose power loop runs over expo_a, against the bounds of the dual form's first spectrum."""
    engine, plan = switches
    sub, rstd, pa, S = _raw_patch_spectra(engine, calls, dev, kind, 1024, dual=False)
    assert calls.count("mc_xc_rows_forward_dual_raw") == 1 and calls.count("mc_xc_cols_forward") == 1
    _raw_patch_check(kind, pa, sub, rstd, (S,), f"1024 {kind} single")


def test_raw_patch_jobs_in_chunks(dev, calls, switches, nan_outputs):
    """WORKSPACE_BYTES lowered to two jobs per chunk: three launches (2 + 2 + 1 jobs), each with its own slice of the
    offsets, the exponents and the per-job subtrahends -- bit for bit the spectra of the one launch."""
    engine, plan = switches
    sub, rstd, pa, whole = _raw_patch_spectra(engine, calls, dev, "u8", 1024, dual=True)
    g = xr.geometry(pa)
    engine.WORKSPACE_BYTES = 2 * g.nkx * g.ny * 8 * 2
    assert engine._chunks(5, g.nkx * g.ny * 8 * 2) == (2, [(0, 2), (2, 2), (4, 1)])
    sub2, rstd2, _, parts = _raw_patch_spectra(engine, calls, dev, "u8", 1024, dual=True)
    assert calls.count("mc_xc_rows_forward_dual_raw") == 3 and calls.count("mc_xc_cols_forward") == 6
    name = "mc_xc_rows_forward_dual_raw"
    assert [a[_arg(name, "njobs")] for a in calls.args[name]] == [2, 2, 1]
    assert np.array_equal(sub, sub2) and rstd == rstd2
    assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1])
    _raw_patch_check("u8", pa, sub, rstd, parts, "1024 u8 dual in chunks")


@pytest.mark.parametrize("kind", ["u8", "i16"])
def test_raw_patch_jobs_group_tail(dev, calls, switches, nan_outputs, kind):
    """The row groups' tail, rounds = min(4, (ny - r16) / 8) with ny % 32 != 0.  ny follows from the window height
    alone (the mask's rows, rounded to the row grouping of 16), and among the heights whose column pass is
    mc_xc_cols_forward only h = 16 has ny % 32 != 0: ny = 16, two rounds in one group; the 1024 x 1024 window of the
    other tests has ny = 800, whole groups of four rounds.  Same jobs, gain, frame brightness and exponents, frames of
    (25, 1039)."""
    engine, plan = switches
    ny = {h: xr.geometry(xr.args(h, 1024)).ny for h in xr.RAW_PATCH_HEIGHTS}
    print(f"raw patch jobs: ny = {ny[1024]} for the (1024, 1024) window, ny = {ny[16]} for the (16, 1024) window")
    assert ny[1024] % 32 == 0 and ny[16] % 32 != 0 and ny[16] % 8 == 0
    sub, rstd, pa, out = _raw_patch_spectra(engine, calls, dev, kind, 16, dual=True)
    _raw_patch_check(kind, pa, sub, rstd, out, f"16 {kind} dual")


# ------------------------------------------------------------------ raw movies


RAW_SHAPES = [(3, 512, 1024), (2, 512, 4096), (2, 96, 5760), (2, 96, 11520)]


def _raw_movie_case(engine, plan, calls, dev, shape, kind, wide_gain=False):
    """One raw movie through engine._global_spectra_raw against the float64 conditioning (raw * gain - sub_f) * rstd
    with the statistics the kernels were given; the bound includes the conditioning term.  `wide_gain`:
    kernel_harness.gain (log-uniform in [0.25, 4]) instead of 1 + 0.05 randn."""
    t, h, w = shape
    g = torch.Generator().manual_seed(h + w + (kind == "u8"))
    if kind == "u8":
        raw = torch.clamp(torch.round(torch.randn(t, h, w, generator=g) * 6 + 40), 0, 255).to(torch.uint8)
    else:
        raw = torch.round(torch.randn(t, h, w, generator=g) * 30 + 1000).to(torch.int16)
    gain = (1.0 + 0.05 * torch.randn(h, w, generator=g)).float()
    if wide_gain:
        gain = kernel_harness.gain(h, w)
    rm = engine.RawMovie(raw.to(dev), gain.to(dev))
    calls.clear()
    S, pl = engine._global_spectra_raw(rm, t // 2, 1.0, xr.B_FACTOR, xr.DEFAULT_BAND)
    torch.cuda.synchronize()
    native = plan.native_rows(pl.geom)
    assert native == (w != 5760 and w != 11520)
    calls.ran("mc_xc_rows_forward_raw" if native else "mc_xcg_rows_forward_raw", _cols_entry(plan, pl.geom),
              absent=("mc_xc_rows_forward", "mc_xcg_rows_forward", "mc_condition_movie"))
    if native:  # the chord table goes to the kernel exactly when the switch is on
        name = "mc_xc_rows_forward_raw"
        assert pl.chord is not None
        assert all((a[_arg(name, "row_chord")] is not None) == bool(engine.USE_ROW_CHORDS) for a in calls.args[name])
    sub = rm.sub.cpu().numpy()
    rstd = float(rm.mean_rstd.cpu()[1])
    v = condition_float64(raw.numpy(), gain.numpy(), sub)
    pa = xr.args(h, w)
    parts = xr.spectra_parts(v, pa, stats=(0.0, 1.0 / rstd))
    mask = xr.tables64(pa)[0]
    bs = []
    for f in range(t):
        cond = np.linalg.norm(conditioning_error(raw[f].numpy(), gain.numpy(), sub[f]) * mask) / np.linalg.norm(v[f] * mask)
        bs.append(xr.spectra_bounds(pa, 0.0, 1.0 / rstd, conditioning=float(cond)))
    what = f"raw {kind} {shape} {'gain [0.25, 4]' if wide_gain else 'gain 1 +- 0.05'} chords={bool(engine.USE_ROW_CHORDS)}"
    r = xr.check_spectra(S, parts, bs, what)
    print(f"RATIO {what} {bs[0]['kinds']} (conditioning {bs[0]['conditioning'] / U:.1f} u of {bs[0]['rel'] / U:.0f} u): "
          f"L2 {r[0]:.3f} bin {r[1]:.3f}")


@pytest.mark.parametrize("kind", ["u8", "i16"])
@pytest.mark.parametrize("shape", RAW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_raw_movies(dev, calls, switches, shape, kind):
    """engine._global_spectra_raw on u8 and i16 counts with a gain reference of 1 +- 0.05: the workgroup kernel (1024
    columns), the wave-per-row kernel (4096, with its row chords) and the direct 2880- and 5760-point rows (5760 and
    11520 columns, the K3 formats: mc_xcg_rows_forward_raw)."""
    engine, plan = switches
    assert engine.USE_ROW_CHORDS
    _raw_movie_case(engine, plan, calls, dev, shape, kind)
    assert calls.count("mc_xcg_rows_forward_raw") == (1 if shape[2] in (5760, 11520) else 0)


@pytest.mark.parametrize("kind", ["u8", "i16"])
@pytest.mark.parametrize("shape", RAW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_raw_movies_gain_of_large_dynamic_range(dev, calls, switches, shape, kind):
    """The same movies with kernel_harness.gain, log-uniform in [0.25, 4]: a gain read one row or column off changes
    a sample by a factor, where a gain of 1 +- 0.05 changes it by a few percent."""
    engine, plan = switches
    _raw_movie_case(engine, plan, calls, dev, shape, kind, wide_gain=True)


@pytest.mark.parametrize("wide_gain", [False, True], ids=["gain-near-1", "gain-wide"])
@pytest.mark.parametrize("kind", ["u8", "i16"])
def test_raw_movies_without_row_chords(dev, calls, switches, kind, wide_gain):
    """(2, 512, 4096) with USE_ROW_CHORDS = False: engine._global_spectra_raw hands mc_xc_rows_forward_raw no chord
    table (asserted on the recorded argument, whose position comes from the header), and the wave-per-row kernel
    clamps its loads to the mask's bounding columns instead."""
    engine, plan = switches
    engine.USE_ROW_CHORDS = False
    _raw_movie_case(engine, plan, calls, dev, (2, 512, 4096), kind, wide_gain)
    name = "mc_xc_rows_forward_raw"
    assert calls.count(name) == 1 and calls.args[name][0][_arg(name, "row_chord")] is None


# ------------------------------------------------------------------ map, arg-max, neighbourhood


def _peaks_of(engine, S, cur, ref, pl, dev):
    ci = torch.tensor(cur, dtype=torch.int32, device=dev)
    ri = torch.tensor(ref, dtype=torch.int32, device=dev)
    peaks, shifts, nb = engine._peaks(S, ci, S, ri, pl, want_nbhd=True)
    torch.cuda.synchronize()
    return peaks.cpu().numpy(), shifts.cpu().numpy(), nb.cpu().numpy()


def _map_case(engine, plan, calls, dev, t, h, w, kind, near=None):
    """One input kind of one map case: the kernels' spectra, _peaks over every frame against frame t // 2 plus the
    reference frame against itself, each pair against correlation64 of spectra64.  -> (peaks, worst ratios)."""
    x, pa, parts, pairs = xr.map_reference(t, h, w, kind, near)
    pl = _plan(pa, dev)
    S = _plain_spectra(engine, x, pa, parts, pl, dev)
    ref = t // 2
    cur = [f for f, *_ in pairs] + [ref]
    calls.clear()
    peaks, shifts, nb = _peaks_of(engine, S, cur, [ref] * len(cur), pl, dev)
    worst = [0.0, 0.0, 0.0]
    for i, (f, cc64, _, E) in enumerate(pairs):
        what = f"{(t, h, w)} {kind} frame {f}"
        worst[0] = max(worst[0], xr.check_peak(peaks[i], shifts[i], cc64, E, what))
        worst[1] = max(worst[1], xr.check_neighbourhood(nb[i], cc64, peaks[i], E, what))
        worst[2] = max(worst[2], xr.check_offsets(nb[i], cc64, peaks[i], E, what))
        if kind not in ("noise", "tie"):
            assert int(peaks[i]) == int(np.argmax(cc64)), f"{what}: not the unique float64 maximum"
    # the reference frame against itself: the peak is exactly index 0, the neighbourhood has NaN above and left
    cc_self = xr.correlation64(parts["S"][ref], parts["S"][ref], pa)
    b = xr.spectra_bounds(pa, parts["mean"], parts["std"])
    _, E = xr.map_bounds(pa, b["rel"], b["rel"], cc_self)
    assert int(peaks[-1]) == 0 and tuple(shifts[-1]) == (0.0, 0.0), f"{(t, h, w)} {kind}: self-correlation peaks at {peaks[-1]}"
    xr.check_neighbourhood(nb[-1], cc_self, 0, E, f"{(t, h, w)} {kind} self")
    return peaks, worst


KINDS = ("small", "large", "noise", "tie", "border")  # "tie": two exactly tied maxima, the tolerant branch


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", xr.MAP_SEPARATE, ids=lambda c: "x".join(map(str, c)))
def test_map_separate_kernels(dev, calls, switches, case, kind):
    """K3 + K4 + K6 as separate kernels: mc_xc_cols_inverse + mc_xc_rows_inverse_argmax + mc_xc_peak_neighbourhood on
    256 and 512; the chirp-z engine's mc_xcg_cols_inverse + mc_xcg_rows_inverse + mc_xcg_peak_neighbourhood on
    (100, 120), (121, 135) and (96, 5760)."""
    engine, plan = switches
    t, h, w = case
    _, worst = _map_case(engine, plan, calls, dev, t, h, w, kind)
    if plan.native_width(w) and plan.native_height(h):
        calls.ran("mc_xc_cols_inverse", "mc_xc_rows_inverse_argmax", "mc_xc_peak_neighbourhood", absent=("mc_xc_correlate_argmax",))
    else:
        calls.ran("mc_xcg_cols_inverse", "mc_xcg_rows_inverse", "mc_xcg_peak_neighbourhood", absent=("mc_xc_correlate_argmax",))
    print(f"RATIO map separate {case} {kind}: arg-max {worst[0]:.3f} nb {worst[1]:.3f} parabola {worst[2]:.3f}")


@pytest.mark.parametrize("kind", KINDS + ("near",))
@pytest.mark.parametrize("case", xr.MAP_FUSED, ids=lambda c: "x".join(map(str, c)))
def test_map_fused_near_window_search(dev, calls, switches, case, kind):
    """mc_xc_correlate_argmax (the near-window search; shifts of a quarter frame, peaks beyond the window and pure
    noise reach its device-side fallback over the full map) and the same pairs with FUSED_SEARCH = False through the
    separate kernels: both inside the bounds, and identical peaks on the planted cases.  'near': peaks in the last
    searched row of the near window, the first row beyond it, the last stored row and the first not stored, from
    mc_xc_near_rows (stored rows = searched rows + guard rows)."""
    from torch_motion_correction_amd import _lib

    engine, plan = switches
    t, h, w = case
    near = int(_lib.load().mc_xc_near_rows(xr.geometry(xr.args(h, w)))) if kind == "near" else None
    assert near is None or 16 < near < h // 2
    engine.FUSED_SEARCH = True
    fused, worst = _map_case(engine, plan, calls, dev, t, h, w, kind, near)
    calls.ran("mc_xc_correlate_argmax", absent=("mc_xc_rows_inverse_argmax", "mc_xc_peak_neighbourhood"))
    print(f"RATIO map fused {case} {kind}: arg-max {worst[0]:.3f} nb {worst[1]:.3f} parabola {worst[2]:.3f}")
    engine.FUSED_SEARCH = False
    separate, worst = _map_case(engine, plan, calls, dev, t, h, w, kind, near)
    calls.ran("mc_xc_cols_inverse", "mc_xc_rows_inverse_argmax", "mc_xc_peak_neighbourhood", absent=("mc_xc_correlate_argmax",))
    print(f"RATIO map separate {case} {kind}: arg-max {worst[0]:.3f} nb {worst[1]:.3f} parabola {worst[2]:.3f}")
    if kind not in ("noise", "tie"):
        assert np.array_equal(fused, separate)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", [(6, 1024, 1024), (5, 256, 256)], ids=lambda c: "x".join(map(str, c)))
def test_shift_table_in_one_chunk_and_in_several(dev, calls, switches, case, fused):
    """engine._shifts_from_spectra scatters the pairs' shifts into the (t, 2) table: in one call of the fused search,
    and -- WORKSPACE_BYTES lowered to two pairs per chunk -- chunk by chunk through the general path.  Either way
    every row is the wrapped admissible peak and the reference frame's row is exactly zero."""
    engine, plan = switches
    t, h, w = case
    engine.FUSED_SEARCH = fused
    x, pa, parts, pairs = xr.map_reference(t, h, w, "small")
    pl = _plan(pa, dev)
    S = _plain_spectra(engine, x, pa, parts, pl, dev)
    g = pl.geom
    tables = []
    for chunk_pairs in (None, 2):
        if chunk_pairs:
            engine.WORKSPACE_BYTES = chunk_pairs * g.nkx * g.H * 8
        calls.clear()
        table = engine._shifts_from_spectra(S, t, t // 2, pl).cpu().numpy()
        torch.cuda.synchronize()
        want_calls = 1 if not chunk_pairs else math.ceil((t - 1) / 2)
        name = "mc_xc_correlate_argmax" if fused and h >= 1024 else "mc_xc_rows_inverse_argmax"
        assert calls.count(name) == want_calls, (name, calls.count(name), want_calls)
        if name == "mc_xc_correlate_argmax":  # the scatter inside the kernel only when one call covers all pairs
            assert (calls.args[name][0][10] is not None) == (chunk_pairs is None)
        assert table.shape == (t, 2) and not table[t // 2].any() and np.signbit(table[t // 2]).sum() == 0
        for f, cc64, _, E in pairs:
            assert tuple(table[f]) == tuple(float(v) for v in xr.shifts64(np.argmax(cc64), (h, w))), (f, table[f])
        tables.append(table)
    assert np.array_equal(tables[0], tables[1])


# ------------------------------------------------------------------ sub-pixel and accumulation


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("case", [(4, 256, 256), (4, 1024, 1024), (3, 100, 120)], ids=lambda c: "x".join(map(str, c)))
def test_parabola_on_planted_fractional_drifts(dev, calls, switches, case, fused):
    """offsets64 of the kernels' 3 x 3 values against offsets64 of the float64 neighbourhood on movies with planted
    fractional drifts (global_refine_reference.planted_movie), within the propagated bound; the offsets themselves
    are real sub-pixel values, not zeros."""
    engine, plan = switches
    t, h, w = case
    engine.FUSED_SEARCH = fused
    dy, dx = [2.3, -1.6, 0.0, 3.45][:t], [-3.7, 0.45, 0.0, 1.25][:t]
    ref = 2
    x, _ = planted_movie(t, h, w, dy, dx, noise=0.3, seed=h + w)
    pa = xr.args(h, w)
    parts = xr.spectra_parts(x, pa)
    b = xr.spectra_bounds(pa, parts["mean"], parts["std"])
    pl = _plan(pa, dev)
    S = _plain_spectra(engine, x, pa, parts, pl, dev)
    cur = [f for f in range(t) if f != ref]
    calls.clear()
    peaks, shifts, nb = _peaks_of(engine, S, cur, [ref] * len(cur), pl, dev)
    native = plan.native_rows(pl.geom)
    calls.ran("mc_xc_correlate_argmax" if fused and h >= 1024 else
              ("mc_xc_peak_neighbourhood" if native else "mc_xcg_peak_neighbourhood"))
    worst, seen = 0.0, 0
    for i, f in enumerate(cur):
        cc64 = xr.correlation64(parts["S"][f], parts["S"][ref], pa)
        _, E = xr.map_bounds(pa, b["rel"], b["rel"], cc64)
        what = f"planted {case} frame {f}"
        xr.check_peak(peaks[i], shifts[i], cc64, E, what)
        assert xr.shifts64(peaks[i], (h, w)) == (round(dy[f] - dy[ref]), round(dx[f] - dx[ref])), what
        xr.check_neighbourhood(nb[i], cc64, peaks[i], E, what)
        worst = max(worst, xr.check_offsets(nb[i], cc64, peaks[i], E, what))
        oy, ox = xr.offsets64(nb[i])
        seen += abs(oy) > 0.05 or abs(ox) > 0.05
        assert abs(oy) <= 0.75 and abs(ox) <= 0.75
    assert seen >= 1
    print(f"RATIO parabola planted {case} fused={fused}: {worst:.3f}")


def _accumulate(dev, peaks, nb, frames, npatch, P, t, ps, thr, flags, field0=None):
    from torch_motion_correction_amd import _lib
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    lib = _lib.load()
    field = (torch.zeros((2, t, npatch)) if field0 is None else torch.from_numpy(np.asarray(field0, dtype=np.float32))).to(dev)
    pk = torch.from_numpy(np.asarray(peaks, dtype=np.int32)).to(dev)
    nbd = torch.from_numpy(np.asarray(nb, dtype=np.float32)).to(dev)
    fr_ = torch.from_numpy(np.asarray(frames, dtype=np.int32)).to(dev)
    check(lib.mc_field_accumulate(ptr(pk), ptr(nbd), ptr(fr_), len(frames), npatch, P, t, float(ps), float(thr), flags,
                                  ptr(field), stream_ptr(dev)), "mc_field_accumulate")
    torch.cuda.synchronize()
    return field.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_field_accumulate_on_hand_built_input(dev, calls, flags):
    """mc_field_accumulate against accumulate64: both flag bits; equal outer samples (the `!=` guard: no offset on
    that axis), NaN outer samples on an interior peak (the comparison is unequal: the offset, and the value, are NaN
    in both), peaks on the border, wrap at P // 2 and P // 2 + 1 (integer and fractional), an outlier just inside the
    threshold and one just outside, nf < t with a non-trivial frame map and a prior field."""
    P, npatch, t, ps = 64, 10, 5, 1.3
    frames = [3, 0, 4]  # nf = 3 < t = 5
    rng = np.random.default_rng(11)
    nf = len(frames)
    peaks = np.zeros(nf * npatch, dtype=np.int64)
    nb = rng.uniform(0.2, 0.8, size=(nf * npatch, 3, 3)).astype(np.float32)
    nb[:, 1, 1] = 1.5 + rng.uniform(0, 0.5, size=nf * npatch).astype(np.float32)
    # frame 3: the wrap on both sides of P // 2, the guards, the border
    peaks[0:10] = [32 * P + 32, 33 * P + 33, 32 * P + 33, 2 * P + 3, 5 * P + 60, 0, 63 * P + 7, 9 * P + 63, 31 * P + 31, 3 * P + 3]
    nb[0, 2, 1], nb[0, 0, 1] = 0.9, 0.3   # position 32 + positive offset: beyond P // 2 -> wraps to negative
    nb[8, 2, 1], nb[8, 0, 1] = 0.9, 0.3   # 31 + positive offset stays below P // 2
    nb[3, 0, 1] = nb[3, 2, 1]             # equal outer samples in y: no y offset
    nb[4, 1, 0] = nb[4, 1, 2]             # equal outer samples in x
    # frame 0: small shifts around (2, -3) and two candidates for rejection; frame 4: every patch the same shift but one
    base = np.array([2 * P + 61] * npatch)
    peaks[10:20] = base
    peaks[10 + 4] = 4 * P + 61
    peaks[10 + 7] = 9 * P + 61
    peaks[20:30] = 5 * P + 5
    peaks[20 + 2] = 6 * P + 5
    field0 = rng.standard_normal((2, t, npatch)).astype(np.float32)
    # thresholds from the float64 z-scores of frame 0's integer rows: one patch just inside, one just outside
    rows0 = np.array([wv if wv <= P // 2 else wv - P for wv in (peaks[10:20] // P).astype(float)])
    z = np.abs(rows0 - np.sort(rows0)[(npatch - 1) // 2]) / rows0.std(ddof=1)
    thr = float(z[7]) * (0.99 if flags & 2 else 1.0)  # patch 7 (z = max) just outside; below, patch 4 just inside
    assert z[4] < thr * 0.9 or not flags & 2
    calls.clear()
    got = _accumulate(dev, peaks, nb, frames, npatch, P, t, ps, thr, flags, field0)
    calls.ran("mc_field_accumulate")
    want, bound = xr.accumulate64(peaks, nb.astype(np.float64), frames, npatch, P, t, ps, thr, flags, field0)
    err = np.abs(got - want)
    touched = bound > 0
    print(f"RATIO mc_field_accumulate flags {flags}: {float((err[touched] / bound[touched]).max()):.3f}")
    assert (err <= bound).all(), (np.argwhere(err > bound)[:5], err.max())
    assert np.array_equal(got[:, [1, 2]], field0[:, [1, 2]].astype(np.float64))  # frames nobody maps to are untouched
    if flags & 1:
        assert want[0, 3, 0] - field0[0, 3, 0] < 0 < want[0, 3, 8] - field0[0, 3, 8]  # the wrap of a fractional position
        assert want[0, 3, 3] - field0[0, 3, 3] == pytest.approx(2 * ps, abs=1e-6)     # the guard: integer row kept
    if flags & 2:
        assert want[0, 0, 7] - field0[0, 0, 7] != pytest.approx(9 * ps) and want[0, 0, 4] - field0[0, 0, 4] == pytest.approx(4 * ps, abs=0.5)


def test_field_accumulate_nan_outer_samples(dev, calls):
    """An interior peak whose outer samples are NaN: `v2 != v0` holds, the offset is NaN, and NaN is what the
    contract gives for that patch (mc_xc_peak_neighbourhood only writes NaN for border peaks, which the kernel
    excludes by the peak's position, as the reference does); every other patch is unaffected."""
    P, npatch, t = 48, 4, 2
    peaks = np.array([5 * P + 5, 0, 6 * P + 47, 7 * P + 7])
    nb = np.full((4, 3, 3), 0.5, dtype=np.float32)
    nb[:, 1, 1] = 2.0
    nb[0, 0, 1] = np.nan
    nb[1], nb[2] = np.nan, np.nan
    nb[1, 1, 1] = nb[2, 1, 1] = 2.0
    nb[3, 2, 1] = 0.7
    got = _accumulate(dev, peaks, nb, [1], npatch, P, t, 2.0, 3.0, 1)
    want, bound = xr.accumulate64(peaks, nb.astype(np.float64), [1], npatch, P, t, 2.0, 3.0, 1)
    calls.ran("mc_field_accumulate")
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got[0, 1, 0]) and not np.isnan(got[1, 1, 0])
    ok = ~np.isnan(want)
    assert (np.abs(got - want)[ok] <= bound[ok]).all()
    assert got[0, 1, 1] == 0.0 and got[1, 1, 2] == -2.0 and got[0, 1, 2] == 12.0
