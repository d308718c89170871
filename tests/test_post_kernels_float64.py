"""The small kernels every patch estimate and every field warp passes through, against the float64 definitions of
tests/post_reference.py: mc_xc_ref_mean_except_current fed by lattice.leave_one_out_schedule (schedule and kernel checked
together, against the (t, t) table itself), mc_field_smooth_center (every window, both routes, the mean subtraction, one
to three trips of the series loop, in place), spline.axis_taps with mc_spline_lattice / mc_spline_points
(csrc/field_tables.hip: spline_lattice_kernel, spline_points_kernel) through
engine.spline_lattice / engine.spline_points and the four public routes on top of them, and the plan's tables
mc_circle_mask and mc_xc_filter called directly.  Every output goes into a NaN-filled buffer (the engine's own
allocations through the `nan_empty` fixture), no element, frame or bin is left out of a comparison, and every test
asserts which entry points of libmcorr ran.

Bounds: post_reference's docstring has the derivations; none is fitted to a kernel's output.  The smoothing bound
carries one term more than the three the issue behind this file lists (the average of the roundings of the smoothed
values, which enters the mean): the contract evaluated on the CPU is outside the three-term sum, see post_reference B.

Worst measured error / bound per kernel and case group (`RATIO ...` lines, run with -s); the fp32 CPU oracle's own
ratio over the same bounds (tests/test_post_reference_host.py, host run) is in the last column.  The kernels' column
is from one run on an MI355X.

                                                              kernels     fp32 CPU oracle
  ref_mean_except_current, schedules t = 2, 3, 8              0.881       0.275 (t = 2: 0.881 for the fp32 replay)
  ref_mean_except_current, schedules t = 52, 60 (eviction)    0.052       0.070
  ref_mean_except_current, hand-made tables                   0.488       0.282
  field_smooth_center, N(0, 1)                                1.000       1.000 (0.9996: the mean's rounding alone)
  field_smooth_center, N(1000, 1) and the grid field          0.513       0.513
  spline lattice, Catmull-Rom / B-spline                      0.210 / 0.152   0.210 / 0.177
  spline points, Catmull-Rom / B-spline                       0.142 / 0.103   0.122 / 0.124
  circle mask, ring pixels                                    0.399       0.388
  xc filter                                                   0.437       0.432
  public routes (at_t, evaluate, resample, frame_lattices)    0.132

The smoothing rows reach the bound because the kernel and the CPU stand-in do the same three operations (double sum,
one rounding of the mean, one fp32 difference): where |y - mean| is tiny the bound is the mean's rounding alone, and
0.9996 of it is used.  No kernel is outside its bound and none was changed.  On the MI355X the file's 92 tests take
2.2 s in all, the slowest 0.2 s.

Mutations (arithmetic only; each built and run once on the MI355X: new tests of this file that fail / older tests that
fail, the older tests being those of tests/test_gpu_parity.py and tests/test_host.py on these kernels, 50 in all):

  ref_mean_except_current: the reset of d on a rebuild dropped                      10 / 1
  ref_mean_except_current: the first listed member of frame 2 skipped               14 / 11
  field_smooth_center: klo = -half for even windows too                             16 / 1
  field_smooth_center: the mean accumulated in fp32 per thread                       5 / 0
  axis_taps: the hi fold restarted from `basis` (drops what the lo fold added)      21 / 15
  xc_filter_fill: (H + 1) / 2 replaced by H / 2                                      1 / 0
  axis_taps: the hi fold reading the already-folded `w[hi, 3]` instead of `basis`    equivalent: the lo fold never writes
      tap 3, the tables are bit-identical (checked on the host on axes of 1, 2, 3, 5 and 40 samples)
  mask_fill: the right clamp removed                                                 equivalent: 0 / 0.  x <= w - 1 <= right,
      so max(x - right, 0) = 0 with the clamp and without it; the same holds for the left clamp.  Both are dead code.

The fp32 mean is caught on the N(0, 1) fields of 127 patches and more (a mean near 0 leaves a small bound) and, at mean
1000, by the 'grid1000' field alone (also in place): on N(1000, 1) its error is 0.06 bounds.  The sign rule is caught by the one case whose band keeps row (H - 1) / 2 of an odd H; with the default band
that row is never kept and the rule cannot matter.
"""

import numpy as np
import pytest
import torch

import post_reference as pr
from kernel_harness import calls, nan, nan_empty  # noqa: F401

pytestmark = pytest.mark.gpu

U = pr.U
F32 = np.float32


def _close(got, want, bound, what):
    """Every element finite and within its bound -> worst error / bound (elements whose bound is 0 must be exact)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} elements unwritten or non-finite"
    err = np.abs(got - want)
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements outside the bound, first {np.argwhere(bad)[0].tolist()}: "
                           f"off by {err[bad][0]:.3e}, bound {bound[bad][0]:.3e}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


# ------------------------------------------------------------------ A. reference spectra


def _table(name):
    from torch_motion_correction_amd import lattice

    if isinstance(name, int):
        return lattice.mask_schedule(name, "mean_except_current", name // 2)[0]
    return pr.hand_table(pr.HAND_TABLES[name])


def _ref_spectra(dev, calls, table, u, v):
    from torch_motion_correction_amd import _lib, lattice
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    lib = _lib.load()
    t, npatch, length, _ = u.shape
    sp, si, sr = lattice.leave_one_out_schedule(table)
    sp, si, sr = (torch.from_numpy(a).to(dev) for a in (sp, si, sr))
    ud, vd = torch.from_numpy(u).to(dev), torch.from_numpy(v).to(dev)
    ref = nan(u.shape, dev)
    calls.clear()
    check(lib.mc_xc_ref_mean_except_current(ptr(ud), ptr(vd), ptr(sp), ptr(si), ptr(sr), ptr(ref), t, npatch, length,
                                            1.0 / (t - 1), stream_ptr(dev)), "mc_xc_ref_mean_except_current")
    torch.cuda.synchronize()
    calls.only("mc_xc_ref_mean_except_current", 1)
    assert torch.equal(ud.cpu(), torch.from_numpy(u)) and torch.equal(vd.cpu(), torch.from_numpy(v))
    return ref.cpu().numpy().reshape(t, npatch * length, 2)


@pytest.mark.parametrize("pair", pr.REF_PAIRS)
@pytest.mark.parametrize("name", pr.SCHEDULE_T + list(pr.HAND_TABLES))
def test_reference_spectra(dev, calls, name, pair):
    """Every frame and element of REF against the table's own definition; the t = 8 schedule at all four sizes (1,
    255, 257 and 3 x 173 complex values), every other table at 3 x 173."""
    table = _table(name)
    t = table.shape[0]
    worst = 0.0
    for npatch, length in (pr.REF_SIZES if name == 8 else pr.REF_SIZES[-1:]):
        u, v = pr.ref_inputs(t, npatch, length, pair)
        want, bound = pr.ref_mean64(pr.to_complex(u), pr.to_complex(v), table)
        got = _ref_spectra(dev, calls, table, u, v)
        worst = max(worst, _close(got, np.stack([want.real, want.imag], axis=-1), bound, f"table {name} {npatch} x {length} {pair}"))
    print(f"RATIO ref_mean_except_current table {name} {pair}: {worst:.3f}")


# ------------------------------------------------------------------ B. smoothing and centring


def _smooth(dev, calls, x, window, subtract_mean, in_place=False):
    from torch_motion_correction_amd import _lib
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    lib = _lib.load()
    _, t, npatch = x.shape
    xd = torch.from_numpy(x).to(dev)
    out = xd if in_place else nan(x.shape, dev)
    calls.clear()
    check(lib.mc_field_smooth_center(ptr(xd), ptr(out), t, npatch, window, subtract_mean, stream_ptr(dev)),
          "mc_field_smooth_center")
    torch.cuda.synchronize()
    calls.only("mc_field_smooth_center", 1)
    if not in_place:
        assert torch.equal(xd.cpu(), torch.from_numpy(x)), "the input was written"
    return out.cpu().numpy()


@pytest.mark.parametrize("subtract_mean", [0, 1])
@pytest.mark.parametrize("npatch", pr.SMOOTH_NPATCH)
def test_smoothing_every_window(dev, calls, npatch, subtract_mean):
    """t = 1 .. 40, window 0 and every window 3 .. t, on the (2, t, npatch) layout with distinct values per series;
    npatch = 129 and 300 take the second and third trip of the 256-thread series loop."""
    assert (2 * npatch > 256) == (npatch in (129, 300)) and (2 * npatch > 512) == (npatch == 300)
    worst = 0.0
    for t in pr.SMOOTH_T:
        x = pr.smooth_field(t, npatch, "unit")
        assert len(np.unique(x.transpose(0, 2, 1).reshape(-1, t), axis=0)) == 2 * npatch  # no two series alike
        for window in pr.smooth_windows(t):
            want, bound = pr.smooth64(x, window, subtract_mean)
            worst = max(worst, _close(_smooth(dev, calls, x, window, subtract_mean), want, bound,
                                      f"t {t} npatch {npatch} window {window} mean {subtract_mean}"))
    print(f"RATIO field_smooth_center npatch {npatch} subtract_mean {subtract_mean} N(0, 1): {worst:.3f}")


@pytest.mark.parametrize("kind", ["mean1000", "grid1000"])
@pytest.mark.parametrize("shape", [(40, 300), (10, 6), (40, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_smoothing_of_a_field_with_a_large_mean(dev, calls, shape, kind):
    """Mean 1000, unit spread, where an fp32 mean shows; 'grid1000' is the field on which fp32 partial sums are
    biased (post_reference.smooth_field; the host file shows the stand-in outside the bound)."""
    t, npatch = shape
    x = pr.smooth_field(t, npatch, kind)
    worst = 0.0
    for window in (0, 3, 4, 5, t):
        for sub in (0, 1):
            want, bound = pr.smooth64(x, window, sub)
            worst = max(worst, _close(_smooth(dev, calls, x, window, sub), want, bound, f"{kind} {shape} window {window} mean {sub}"))
    print(f"RATIO field_smooth_center {kind} {shape}: {worst:.3f}")


@pytest.mark.parametrize("shape", [(1, 1), (5, 6), (40, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_centring_in_place(dev, calls, shape):
    """window = 0, subtract_mean = 1 with field_out == field_in: the form the host permits."""
    t, npatch = shape
    for kind in ("unit", "grid1000"):
        x = pr.smooth_field(t, npatch, kind)
        want, bound = pr.smooth64(x, 0, 1)
        r = _close(_smooth(dev, calls, x, 0, 1, in_place=True), want, bound, f"in place {shape} {kind}")
        print(f"RATIO field_smooth_center in place {shape} {kind}: {r:.3f}")


# ------------------------------------------------------------------ C. spline grids


def _vec(u):
    return torch.from_numpy(np.asarray(u, dtype=F32))


@pytest.mark.parametrize("grid_type", pr.GRID_TYPES)
@pytest.mark.parametrize("shape", pr.SPLINE_GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_spline_lattice(dev, calls, nan_empty, shape, grid_type):
    """engine.spline_lattice on the four query sets of every grid: knots, 0, 1 and their fp32 neighbours ('edge'),
    linspace(0, 1, 33), the 1 / 2 / 33-point mix, and the field warp's lattice (frame times x 10 points per sample)."""
    from torch_motion_correction_amd import engine

    worst = 0.0
    for kind in pr.SPLINE_QUERIES:
        data, q, want, bound = pr.lattice_case(shape, kind, grid_type)
        calls.clear()
        got = engine.spline_lattice(torch.from_numpy(data).to(dev), *map(_vec, q), grid_type)
        torch.cuda.synchronize()
        calls.only("mc_spline_lattice", 1)
        worst = max(worst, _close(got.cpu().numpy(), want, bound, f"lattice {shape} {kind} {grid_type}"))
    print(f"RATIO spline lattice {shape} {grid_type}: {worst:.3f}")


@pytest.mark.parametrize("grid_type", pr.GRID_TYPES)
@pytest.mark.parametrize("shape", pr.SPLINE_GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_spline_points(dev, calls, nan_empty, shape, grid_type):
    """engine.spline_points at 1, 255, 257 and 1000 points: the eight corners of the cube, uniform points and points
    on knots and beside them."""
    from torch_motion_correction_amd import engine

    worst = 0.0
    for n in pr.POINT_COUNTS:
        data, pts, want, bound = pr.points_case(shape, n, grid_type)
        calls.clear()
        got = engine.spline_points(torch.from_numpy(data).to(dev), torch.from_numpy(pts), grid_type)
        torch.cuda.synchronize()
        calls.only("mc_spline_points", 1)
        worst = max(worst, _close(got.cpu().numpy(), want, bound, f"points {shape} n {n} {grid_type}"))
    print(f"RATIO spline points {shape} {grid_type}: {worst:.3f}")


def test_tap_cache_tells_two_coordinate_vectors_of_equal_length_apart(dev, calls, nan_empty):
    from torch_motion_correction_amd import engine

    shape = (3, 7, 6, 9)
    data = pr.spline_grid(shape)
    d = torch.from_numpy(data).to(dev)
    a = pr.lin(33)
    b = (a.astype(np.float64) ** 2).astype(F32)
    for q in ((a, a, a), (b, b, b), (a, b, a)):
        want, bound = pr.spline_lattice64(data, *q, "bspline")
        calls.clear()
        got = engine.spline_lattice(d, *map(_vec, q), "bspline")
        torch.cuda.synchronize()
        calls.only("mc_spline_lattice", 1)
        _close(got.cpu().numpy(), want, bound, "tap cache")


def test_public_routes_over_the_spline_kernels(dev, calls, nan_empty):
    """evaluate_deformation_field_at_t, evaluate_deformation_field, resample_deformation_field (Catmull-Rom) and
    engine.frame_lattices (the field warp's B-spline lattice) against the same definition."""
    import torch_motion_correction_amd as mc
    from torch_motion_correction_amd import engine

    shape = (2, 3, 2, 5)
    data = pr.spline_grid(shape)
    field = torch.from_numpy(data)
    for grid_type in pr.GRID_TYPES:
        tq = F32(0.37)
        want, bound = pr.spline_lattice64(data, [tq], pr.lin(7), pr.lin(11), grid_type)
        calls.clear()
        got = mc.evaluate_deformation_field_at_t(field.to(dev), float(tq), (7, 11), grid_type=grid_type)
        calls.only("mc_spline_lattice", 1)
        r1 = _close(got.cpu().numpy(), want[:, 0], bound[:, 0], f"at_t {grid_type}")
        _, pts, want, bound = pr.points_case(shape, 257, grid_type)
        calls.clear()
        got = mc.evaluate_deformation_field(field.to(dev), torch.from_numpy(pts).reshape(1, 257, 3), grid_type=grid_type)
        calls.only("mc_spline_points", 1)
        r2 = _close(got.cpu().numpy()[0], want, bound, f"evaluate {grid_type}")
        print(f"RATIO public routes {grid_type}: at_t {r1:.3f} evaluate {r2:.3f}")
    want, bound = pr.spline_lattice64(data, pr.lin(9), pr.lin(4), pr.lin(3), "catmull_rom")
    calls.clear()
    got = mc.resample_deformation_field(field.to(dev), (9, 4, 3))
    calls.only("mc_spline_lattice", 1)
    r3 = _close(got.cpu().numpy(), want, bound, "resample")
    _, q, want, bound = pr.lattice_case(shape, "dense", "bspline")
    calls.clear()
    got = engine.frame_lattices(field.to(dev), shape[1], "bspline")
    torch.cuda.synchronize()
    calls.only("mc_spline_lattice", 1)
    r4 = _close(got.cpu().numpy(), want.transpose(1, 0, 2, 3), bound.transpose(1, 0, 2, 3), "frame_lattices")
    print(f"RATIO public routes: resample {r3:.3f} frame_lattices {r4:.3f}")


# ------------------------------------------------------------------ D. plan tables


@pytest.mark.parametrize("case", pr.MASK_CASES, ids=lambda c: "-".join(f"{v:g}" for v in c))
def test_circle_mask(dev, calls, case):
    """mc_circle_mask directly: inside pixels exactly 1, pixels beyond the ring exactly 0, ring pixels within 6u."""
    from torch_motion_correction_amd import _lib
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    h, w, r, s = case
    inside, ring, value, halfw = pr.mask64(*case)
    mask = nan((h, w), dev)
    hw = torch.full((h,), -7, dtype=torch.int32, device=dev)
    calls.clear()
    check(_lib.load().mc_circle_mask(ptr(mask), ptr(hw), h, w, float(r), float(s), stream_ptr(dev)), "mc_circle_mask")
    torch.cuda.synchronize()
    calls.only("mc_circle_mask", 1)
    got = mask.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and np.array_equal(hw.cpu().numpy(), halfw)
    assert (got[inside] == 1).all(), "an inside pixel is not exactly 1"
    assert (got[~inside & ~ring] == 0).all(), "a pixel beyond the ring is not exactly 0"
    if not inside.any():
        assert not got.any()
    if ring.any():
        err = np.abs(got - value)[ring]
        print(f"RATIO circle mask {case}: {err.max() / pr.MASK_RING_BOUND:.3f}")
        assert err.max() <= pr.MASK_RING_BOUND, f"ring off by {err.max():.3e}"


@pytest.mark.parametrize("case", pr.FILTER_CASES, ids=lambda c: c[5])
def test_xc_filter(dev, calls, case):
    """mc_xc_filter directly on the plan's geometry: excluded bins exactly 0, kept bins within (12 |E| + 2) u."""
    from torch_motion_correction_amd import _lib, plan
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    H, W, ps, B, band, what = case
    low, high = plan.band_limits(band, ps)
    g = plan.xc_geometry(H, W, high, min(H, W) / 4, min(H, W) / 8)
    kept, value, bound = pr.filter64(W, H, g.nkx, g.kyp, g.kyn, low, high, B, ps)
    filt = nan((g.nkx, g.nky), dev)
    calls.clear()
    check(_lib.load().mc_xc_filter(ptr(filt), g, low, high, float(B), float(ps), stream_ptr(dev)), "mc_xc_filter")
    torch.cuda.synchronize()
    calls.only("mc_xc_filter", 1)
    got = filt.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert np.array_equal(got != 0, kept), f"band decisions differ at {np.argwhere((got != 0) != kept)[:4].tolist()}"
    r = _close(got, value, bound, f"filter {what}")
    if B == 0:
        assert (got[kept] == 1).all()
    print(f"RATIO xc filter {what}: {r:.3f}")
