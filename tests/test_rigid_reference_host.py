"""Host checks of what tests/test_rigid_kernels_float64.py stands on (tests/rigid_reference.py): the gather-based
float64 resampler equals the dense one, the rigid kernels' two-offset invariant holds for the reference's fp32
coordinate chain, and the shift tables of the GPU cases cover what the kernels specialise on."""

import numpy as np
import pytest

from rigid_reference import (KERNEL_CASES, KERNEL_SHIFT_POOL, RECENTRE_INTS, RECENTRE_SHIFTS, _cubic_weights,
                             _grid_chain, cubic_weight_error, kernel_case_shifts, kernel_shift_coverage,
                             rigid_resample, rigid_resample_gather)

F32 = np.float32


# ------------------------------------------------------------------ the two resamplers agree


def _agreement_shifts(h, w):
    return [(2.37, -5.61), (-40.5, 77.25), (0.0, 0.0), (0.5, -0.5), (3.0, -7.0), (-1.0, 1.0),  # fractional, integer
            (3 + 2.0 ** -12, -(2.0 ** -11)), (1e-7, -1e-7),
            (h - 1, -(w - 1)), (-(h - 1), w - 1), (h - 1.5, -(w - 1.5)), (h - 0.5, 2.25),  # exactly +-(n - 1)
            (h, 0.25), (-1.5, -w), (3.0 * h + 0.5, -2.0 * w), (-(h + 40.25), w + 300.5)]  # larger than the frame


@pytest.mark.parametrize("shape", [(130, 250), (64, 96), (33, 47), (5, 8), (2, 3), (128, 31)])
def test_gather_resampler_equals_the_dense_one(shape):
    """Output to 1e-12 of max|frame|, identical zero pattern, and a magnitude that is >= the dense resampler's
    (which merges the taps that clip to one border sample before the absolute values; `>=` up to the rounding of
    two float64 sums of 16 terms taken in different orders, 1e-13 of max|frame|) and equal to it where no tap
    clips."""
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    frame = (rng.standard_normal((h, w)) * 2 + 5).astype(F32)
    assert not (frame == 0).any()
    top = float(np.abs(frame).max())
    for sy, sx in _agreement_shifts(h, w):
        sy, sx = F32(sy), F32(sx)
        out_d, mag_d = rigid_resample(frame, sy, sx)
        err = rng.random((h, w))
        out_g, mag_g, err_g = rigid_resample_gather(frame, sy, sx, extra=(err,))
        case = (shape, float(sy), float(sx))
        assert np.array_equal(out_d == 0, out_g == 0), case
        assert float(np.abs(out_d - out_g).max()) <= 1e-12 * top, (case, float(np.abs(out_d - out_g).max()))
        assert float((mag_d - mag_g).max()) <= 1e-13 * top, (case, float((mag_d - mag_g).max()))
        assert np.array_equal(mag_g == 0, out_d == 0), case  # no input sample is zero
        assert bool((mag_g >= np.abs(out_g) - 1e-13 * top).all()), case
        # the extra map goes through the same absolute weights: a constant map c gives c * sum_ij |wy_i| |wx_j|
        _, ones_mag, ones_err = rigid_resample_gather(np.ones((h, w)), sy, sx, extra=(np.full((h, w), 3.0),))
        assert np.allclose(ones_err, 3.0 * ones_mag, rtol=1e-14, atol=0), case
        assert bool((err_g <= ones_mag * (1 + 1e-14)).all()) and bool((err_g >= 0).all()), case
        interior = np.zeros((h, w), dtype=bool)
        if abs(float(sy)) < h - 8 and abs(float(sx)) < w - 8 and h > 16 and w > 16:  # taps that do not clip
            y0, y1 = max(2, 2 - int(np.floor(sy))), min(h - 3, h - 3 - int(np.ceil(sy)))
            x0, x1 = max(2, 2 - int(np.floor(sx))), min(w - 3, w - 3 - int(np.ceil(sx)))
            interior[y0:y1, x0:x1] = True
            assert float(np.abs(mag_d - mag_g)[interior].max(initial=0.0)) <= 1e-13 * top, case


def test_gather_resampler_magnitude_counts_clipped_taps_apart():
    """At the border two taps with weights of opposite sign clip to the same sample: the kernels add the two
    products, the dense operator adds the two weights first.  The gather magnitude is strictly larger there."""
    frame = np.full((16, 16), 5.0, dtype=F32)
    _, mag_d = rigid_resample(frame, F32(0.5), F32(0.5))
    _, mag_g = rigid_resample_gather(frame, F32(0.5), F32(0.5))
    assert mag_g[0, 0] > mag_d[0, 0] * 1.05 and mag_g[8, 8] == pytest.approx(mag_d[8, 8], rel=1e-14)


def test_cubic_weight_error_bounds_an_fp32_evaluation():
    """cubic_weight_error against ATen's Horner forms evaluated operation by operation in fp32 (numpy, no fusing), for
    two million random fractions and the fractions 2^-k and 1 - 2^-k: the bound holds, is within 2x of the worst
    error seen for the far taps, and that error is far beyond 8 ulp of the weight itself -- a far weight of ~2e-4
    carries an absolute error of ~1e-6 -- which is why the kernels' frame bound has an absolute weight term."""
    k = np.arange(1, 24)
    t = np.concatenate([np.random.default_rng(0).random(2_000_000), 2.0 ** -k, 1 - 2.0 ** -k, [0.0]]).astype(F32)
    A, c1, c2, c4, c5, c8 = (F32(v) for v in (-0.75, 1, 2, 4, 5, 8))

    def far(x):
        return ((A * x - c5 * A) * x + c8 * A) * x - c4 * A

    def near(x):
        return ((A + c2) * x - (A + F32(3))) * x * x + c1

    w32 = np.stack([far(t + c1), near(t), near(c1 - t), far(c2 - t)], axis=-1)
    assert w32.dtype == F32
    w64 = _cubic_weights(t)
    err, bound = np.abs(w32.astype(np.float64) - w64), cubic_weight_error(t)
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float((err / bound)[:, 0].max()) > 0.5 and float((err / bound)[:, 3].max()) > 0.5
    assert float((err[:, 0] / (8 * 2.0 ** -24 * np.abs(w64[:, 0]) + 1e-300)).max()) > 100


# ------------------------------------------------------------------ the two-offset invariant

INVARIANT_SIZES = (2, 3, 5, 33, 64, 130, 256, 516, 959, 1000, 4092, 4096, 5760, 8184, 8192, 11520, 16384)


def _invariant_shifts(n):
    rng = np.random.default_rng(n)
    sh = list(rng.uniform(-40, 40, 300))
    for k in (-33, -8, -1, 0, 1, 3, 32, 513):
        for e in (0, 1e-7, -1e-7, 1e-4, -1e-4, 0.5, -0.5, 1 - 1e-6):
            sh.append(k + e)
    sh += [n - 1, -(n - 1), n - 1.5, n, -n, 3 * n]
    return np.array(sh, dtype=F32)


@pytest.mark.parametrize("n", INVARIANT_SIZES)
def test_floor_offset_takes_two_adjacent_values(n):
    """What rigid_base / rigid_weights (csrc/warp_rigid.hip) assume: with u = the fp32 grid chain of c = fp32(p + s) and
    S = min over ALL p of floor(u(p)) - p (rigid_base's reduction), d = floor(u(p)) - p - S is 0 or 1 for every p
    whose coordinate lies inside [0, n - 1].  rigid_weights writes all-zero weights for any other d, so a
    violation would be rows or columns silently zeroed by the kernels."""
    p = np.arange(n, dtype=F32)
    bad = []
    for s in _invariant_shifts(n):
        c = (p + s).astype(F32)
        inside = (c >= F32(0)) & (c <= F32(n - 1))
        fl = np.floor(_grid_chain(c, n))
        lim = F32(3.0) * F32(n) + F32(16.0)  # rigid_base's clamp (a guard: never active for these shifts)
        off = np.clip(fl - p, -lim, lim).astype(np.int64)
        d = off - off.min()
        if inside.any() and not bool(((d[inside] == 0) | (d[inside] == 1)).all()):
            bad.append((float(s), sorted({int(v) for v in d[inside]})))
    assert not bad, (n, bad[:10])


# ------------------------------------------------------------------ the GPU cases' shifts


def _used(kernel, cases=None):
    ys, xs = [], []
    for case in (KERNEL_CASES[kernel] if cases is None else cases):
        sh = kernel_case_shifts(*case)
        ys += list(sh[:, 0])
        xs += list(sh[:, 1])
    return ys, xs


def test_shift_pool_covers_what_the_kernels_specialise_on():
    assert kernel_shift_coverage(KERNEL_SHIFT_POOL, x_axis=True) == []
    for v in KERNEL_SHIFT_POOL:
        assert float(F32(v)) == v or abs(v - round(v, 2)) < 1e-12  # the tiny fractions are exact in fp32


@pytest.mark.parametrize("kernel", sorted(KERNEL_CASES))
def test_kernel_cases_cover_signs_fractions_and_residues(kernel):
    """Per kernel and per axis the shifts its cases run contain both signs, a fraction of exactly 0.5, a fraction
    below 2^-10, an integer and -- x axis -- integer parts of every residue mod 4; the raw i16 cases (all raw cases
    but the 4096^2 one) on their own too."""
    ys, xs = _used(kernel)
    assert kernel_shift_coverage(ys, x_axis=False) == []
    assert kernel_shift_coverage(xs, x_axis=True) == []
    if kernel == "warp_rigid_raw":
        ys, xs = _used(kernel, KERNEL_CASES[kernel][:-1])
        assert kernel_shift_coverage(ys, x_axis=False) == [] and kernel_shift_coverage(xs, x_axis=True) == []


@pytest.mark.parametrize("kernel", sorted(KERNEL_CASES))
def test_kernel_cases_reach_the_edges(kernel):
    """Every case has a shift >= n (an all-zero frame), the shift that leaves one row and one column, and a shift
    beyond the tile wherever the frame allows one; the number of shifts is a multiple of t."""
    for case in KERNEL_CASES[kernel]:
        t, h, w = case[:3]
        sh = kernel_case_shifts(*case).astype(np.float64)
        assert sh.shape[0] % t == 0
        assert ((np.abs(sh[:, 0]) >= h) | (np.abs(sh[:, 1]) >= w)).any(), case
        assert ((sh[:, 0] == h - 1.5) & (sh[:, 1] == -(w - 1.5))).any(), case
        live = (np.abs(sh[:, 0]) < h - 1) & (np.abs(sh[:, 1]) < w - 1)
        if h >= 64:
            assert (live & (np.abs(sh[:, 0]) > 32)).any(), case
        if w >= 1024:
            assert (live & (np.abs(sh[:, 1]) > 512)).any(), case
        assert (live & (np.abs(sh[:, 1]) > 64)).any(), case


def test_recentring_sequence_jumps_as_stated():
    ints = np.array(RECENTRE_INTS)
    assert np.array_equal(np.floor(RECENTRE_SHIFTS.astype(np.float64)).astype(int), ints)
    dy, dx = np.diff(ints[:, 0]), np.diff(ints[:, 1])
    for axis in (dy, dx):
        assert {5, 9, -9, -20, 20} <= {int(v) for v in axis}
    assert ((dy != 0) & (dx != 0)).any() and ((dy != 0) & (dx == 0)).any() and ((dy == 0) & (dx != 0)).any()
    assert tuple(ints[0]) == tuple(ints[-1])
    # beyond the spare 8 rows / columns (+-4 around the first window) more than once, and within them too
    assert (np.abs(dy) > 8).sum() >= 2 and (np.abs(dx) > 8).sum() >= 2 and (np.abs(dy) == 5).any()
