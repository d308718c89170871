"""Host checks of the rigid-warp shift rule and of the float64 resampler the GPU route tests
(tests/test_rigid_routes.py) compare against.  No GPU needed.

The canonical shift rule (tests/rigid_reference.py): shifts_px = fp32(L) / fp32(ps), correctly rounded."""

import numpy as np
import pytest
import torch

import oracle
from oracle import thirdparty_semantics as tp
from rigid_reference import (EXACT_RECIPROCAL, FRAME_SPACINGS, LARGE_SHIFTS, PIPELINE_SPACINGS, RAW_SPACINGS,
                             SMALL_SHIFTS, TABLE_SPACINGS, canonical_shift, differing_shifts, reciprocal_shift,
                             rigid_resample, rigid_resample_stack, row_dropping_shifts)


@pytest.mark.parametrize("ps", [0.83, 1.06, 1.3, 1.35, 1.37, 2.5, 1.0])
def test_canonical_rule_is_what_the_cpu_reference_computes(ps):
    """The oracle's get_pixel_shifts divides a CPU fp32 tensor by the Python float ps: true division, i.e. the
    correctly rounded fp32 quotient -- numpy's float32 division."""
    s = np.arange(-200, 201)
    L = torch.from_numpy(s.astype(np.float32)) * ps
    assert np.array_equal((L / ps).numpy(), canonical_shift(s, ps))
    assert np.array_equal(L.numpy(), s.astype(np.float32) * np.float32(ps))


def test_the_two_roundings_differ_where_the_issue_says():
    s = np.arange(-200, 201)
    count = lambda ps: int((canonical_shift(s, ps) != reciprocal_shift(s, ps)).sum())  # noqa: E731
    assert [count(ps) for ps in (0.83, 1.06, 1.3, 1.35)] == [86, 36, 66, 54]
    assert [count(ps) for ps in (0.5, 1.37, 2.0, 1.0)] == [0, 0, 0, 0]
    # the integer itself is the true quotient; the reciprocal product sits just below it for negative s
    assert row_dropping_shifts(range(-12, 13), 0.83) == [-12, -11, -10, -6, -5, -3]
    assert np.array_equal(canonical_shift([-3, -5, -6], 0.83), np.float32([-3, -5, -6]))


@pytest.mark.parametrize("ps", sorted(set(TABLE_SPACINGS + FRAME_SPACINGS + PIPELINE_SPACINGS + RAW_SPACINGS)))
def test_gpu_cases_cover_the_rounding_difference(ps):
    """Guard of the GPU tests' cases: at every spacing != 1 whose reciprocal is inexact the shift set contains
    integers where the two roundings differ; at 0.83 (used by every GPU group) it contains negative ones where
    the reciprocal product is MORE negative -- the case that zeroes a border row or column the reference keeps.
    At 1.06, 1.3 and 1.35 fp32(1/ps) < 1/ps, so the reciprocal never errs towards the border for s < 0; there
    the differing shifts move the sample by a coordinate ulp and change floor() at the first row/column."""
    shifts = SMALL_SHIFTS + LARGE_SHIFTS
    if ps in EXACT_RECIPROCAL:
        assert differing_shifts(range(-200, 201), ps) == []
        return
    assert len(differing_shifts(shifts, ps)) >= 4
    if ps == 0.83:
        assert {-3, -5, -6} <= set(row_dropping_shifts(shifts, ps))
    assert 0.83 in FRAME_SPACINGS and 0.83 in PIPELINE_SPACINGS and 0.83 in RAW_SPACINGS


def test_float64_resampler_zero_rule_and_integer_shift():
    """An exact integer shift is a translation: interior values are the input's up to the fp32 round trip of the
    coordinate through grid_sample's normalisation (a few ulp of the index), rows/columns whose coordinate
    p + s leaves [0, n-1] are exactly zero, the one at c = 0 is kept.  A coordinate just below zero
    (-3 - 2.4e-7, the reciprocal's value at ps = 0.83) drops row 3."""
    g = torch.Generator().manual_seed(3)
    fr = (torch.randn(24, 30, generator=g) * 2 + 5).double().numpy()
    out, _ = rigid_resample(fr, np.float32(-3), np.float32(4))
    assert np.all(out[:3] == 0) and np.all(out[:, 26:] == 0)
    assert np.abs(out[3:, :26] - fr[:21, 4:]).max() <= 1e-5 * np.abs(fr).max()
    assert np.all(out[3:, :26] != 0)
    out2, _ = rigid_resample(fr, reciprocal_shift(-3, 0.83), np.float32(4))
    assert np.all(out2[:4] == 0) and np.all(out2[4:, :26] != 0)


@pytest.mark.parametrize("shape,ps", [((3, 40, 52), 1.0), ((3, 33, 47), 0.83), ((2, 64, 48), 1.3)])
def test_float64_resampler_matches_the_oracle(shape, ps):
    """Against oracle.correct_motion on a rigid field (fractional and integer shifts), away from the knife edge:
    the oracle upsamples the constant lattice bicubically, so its per-pixel shift is L (1 +- ~2e-6) / ps and pixels
    whose coordinate lies within 1e-3 px of the border may fall either way ("Knife-edge pixels").
    Elsewhere the two agree to the oracle's fp32 arithmetic (1e-5 of the range).  And against the oracle's own
    sampling rule (tp.sample_image_2d) at the exact fp32 shift, with no mask at all: the zero pattern is equal."""
    t, h, w = shape
    g = torch.Generator().manual_seed(h * w)
    st = torch.randn(t, h, w, generator=g) * 2 + 5
    for px in (torch.randn(t, 2, generator=g) * 4, torch.tensor([[-3.0, 5.0], [-5.0, -6.0], [2.0, -3.0]])[:t]):
        field = (px * ps).T[:, :, None, None].contiguous()
        ref = oracle.correct_motion(st, field, ps)
        lat = [oracle.evaluate_deformation_field_at_t(field, ft, (10, 10), "catmull_rom")
               for ft in torch.linspace(0, 1, steps=t)]
        sh = np.stack([(lt[:, 0, 0] / ps).numpy() for lt in lat]).astype(np.float32)
        got, _ = rigid_resample_stack(st.numpy(), sh)
        grid = tp.coordinate_grid((h, w))
        knife = torch.zeros(t, h, w, dtype=torch.bool)
        for f in range(t):
            c = grid + oracle.get_pixel_shifts(st[f], ps, lat[f], grid)
            near = lambda v, n: (v.abs() < 1e-3) | ((v - (n - 1)).abs() < 1e-3)  # noqa: E731
            knife[f] = near(c[..., 0], h) | near(c[..., 1], w)
        d = np.abs(got - ref.double().numpy())
        d[knife.numpy()] = 0
        assert d.max() <= 1e-5 * float(ref.abs().max()), d.max()
        for f in range(t):
            exact = tp.sample_image_2d(st[f], grid + torch.from_numpy(sh[f]), interpolation="bicubic").double().numpy()
            assert np.array_equal(exact == 0, got[f] == 0)
            assert np.abs(exact - got[f]).max() <= 1e-5 * float(np.abs(exact).max())
