"""tests/field_reference.py checked on the host: against the fp32 torch port of the reference project
(oracle.correct_motion / oracle.get_pixel_shifts), against the rigid resampler for constant lattices, the identity
for the zero lattice, its shift bound against operation-by-operation fp32 evaluations -- and what the cases of
tests/test_field_kernels_float64.py reach, derived from the documented dispatch rules alone."""

import numpy as np
import pytest
import torch

import oracle
from field_reference import (ACCUM_CASES, ACCUM_RUNS, ACCUM_SPACINGS, accumulate_lattices, CASE_STORAGE, FAMILIES, FIELD_CASES, TILE_H, TILE_W, axis_tables, case_launches,
                             case_lattices, coordinate_candidates, dot4_f32, e_table, family_lattice, field_reference,
                             route_of, shift_interval, tile_plan)
from rigid_reference import F32, _grid_chain, rigid_resample_gather


def _frames(t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(t, h, w, generator=g) * 2 + 5


@pytest.mark.parametrize("ps", [1.0, 0.83])
@pytest.mark.parametrize("grid_type", ["catmull_rom", "bspline"])
def test_reference_contains_the_fp32_oracle(grid_type, ps):
    """The torch port computes the same chain in fp32 in ATen's own operation order: its shifts lie in the
    reference's interval widened by the x pass' rounding (ATen forms it itself, shift_interval(x_pass_error)), its
    frames within the reference's bound of a candidate, with the zero and on-border rules."""
    t, h, w = 2, 37, 45
    st = _frames(t, h, w, 1)
    field = torch.randn(2, 2, 1, 2, generator=torch.Generator().manual_seed(2)) * 3
    lat = np.stack([oracle.evaluate_deformation_field_at_t(field, ft, (10, 20), grid_type).numpy()
                    for ft in torch.linspace(0, 1, steps=t)])
    s, es = shift_interval(lat, h, w, ps, x_pass_error=True)
    grid = torch.stack(torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij"), -1)
    for f in range(t):
        got = oracle.get_pixel_shifts(st[f], ps, torch.from_numpy(lat[f]), grid).double().numpy()
        assert bool((np.abs(got - s[f].transpose(1, 2, 0)) <= es[f].transpose(1, 2, 0)).all())
    ref = field_reference(st.numpy(), lat, ps, x_pass_error=True)
    out = oracle.correct_motion(st, field, ps, grid_type=grid_type).numpy()
    assert ref.check(out, f"oracle {grid_type} {ps}") <= 1.0
    assert ref.zero.any() and not ref.zero.all()


@pytest.mark.parametrize("ps", [1.0, 0.83, 1.3])
def test_constant_lattice_reduces_to_the_rigid_resampler(ps):
    """A constant lattice L: the rigid resampler at the canonical shift fp32(L) / fp32(ps) is one of the values the
    field reference accepts at every pixel (candidate rule, zero and on-border rules)."""
    t, h, w, GH, GW = 4, 33, 70, 3, 4
    st = _frames(t, h, w, 3).numpy().astype(np.float64)
    rng = np.random.default_rng(0)
    names = ("integer", "fraction", "big", "one_row_col")
    lat = np.stack([family_lattice(n, h, w, GH, GW, ps, rng) for n in names])
    lat[2] = (np.array([10.5, -20.25], dtype=F32)[:, None, None] * np.ones((1, GH, GW), dtype=F32) * F32(ps)).astype(F32)
    ref = field_reference(st, lat, ps)
    rigid = np.stack([rigid_resample_gather(st[f], *(lat[f, :, 0, 0] / F32(ps)))[0] for f in range(t)])
    ref.check(rigid, f"rigid ps {ps}")
    assert int(ref.border.sum()) <= t * (h + w)


def test_zero_lattice_returns_the_frame_exactly():
    """Zero lattice: the shift and its bound are exactly 0, there is one candidate per pixel, nothing is zeroed.  At
    33 x 32 the fp32 coordinate chain returns every integer (asserted), the weights are exactly (0, 1, 0, 0) and the
    frame comes back exactly.  At other sizes the chain itself may move an integer coordinate by an ulp or so (the
    reference project's own behaviour, which the kernels reproduce): 33 x 70 only has to lie within the bound."""
    for w in (32, 70):
        st = _frames(2, 33, w, 4).numpy().astype(np.float64)
        ref = field_reference(st, np.zeros((2, 2, 3, 4), dtype=F32), 0.83)
        assert not ref.es.any() and not ref.s.any() and not ref.zero.any() and not ref.border.any()
        assert all(np.array_equal(v, ref.vals[0]) for v in ref.vals)
        ref.check(st, "identity")
        if w == 32:
            for n in (33, w):
                p = np.arange(n, dtype=F32)
                assert bool((_grid_chain(p, n) == p).all())
            assert np.array_equal(ref.vals[0], st)


@pytest.mark.parametrize("ps", [1.0, 0.83, 1.3])
def test_shift_bound_holds_for_fp32_evaluations(ps):
    """dot4 + the division evaluated operation by operation in fp32, with separate roundings and with every
    multiply-add fused: both lie within es of the float64 shift; es is exactly 0 where the E values are, and it is
    no vacuous bound (an evaluation reaches a tenth of it)."""
    h, w, GH, GW = 96, 516, 5, 4
    rng = np.random.default_rng(5)
    lat = np.stack([family_lattice(n, h, w, GH, GW, ps, rng) for n in ("smooth6", "rough", "zero", "fraction")])
    s, es = shift_interval(lat, h, w, ps)
    E = e_table(lat, w)
    ytap, ycoef = axis_tables(h, GH)
    rows = np.stack([E[:, :, ytap[:, k], :] for k in range(4)], -1)  # (t, 2, h, w, 4)
    coef = np.broadcast_to(ycoef[None, None, :, None, :], rows.shape)
    worst = 0.0
    for fused in (False, True):
        q = dot4_f32(coef, rows, fused)
        q = q if ps == 1.0 else (q / F32(ps)).astype(F32)
        assert q.dtype == F32
        d = np.abs(q.astype(np.float64) - s)
        assert bool((d <= es).all()), (fused, float((d - es).max()))
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nan_to_num(d / es, nan=0.0, posinf=0.0).max()))
    assert not es[2].any() and not s[2].any() and bool((es[[0, 1, 3]] > 0).all())
    assert 0.1 <= worst <= 1.0, worst


# ------------------------------------------------------------------ what the GPU cases reach


def _all_cases():
    return [(route, case) for route, cases in FIELD_CASES.items() for case in cases]


def test_every_case_takes_the_route_its_table_entry_names():
    for route, (t, h, w, GH, GW) in _all_cases():
        storage = CASE_STORAGE[route]
        want = "warp_main" if route.startswith("warp_main") else "warp_field2" if route == "warp_field2" else "warp_field3"
        assert route_of(h, w, GH, storage, aligned=route != "warp_main_unaligned") == want, (route, t, h, w, GH, GW)
        assert h <= 96 and w <= 2048 and GH > 1 and GW > 1 and (t <= 3 or h == 33)
    # the unaligned case is a field3 shape but for the pointer, and what the entry points refuse is refused here
    assert route_of(33, 260, 2, "f32") == "warp_field3" and route_of(33, 260, 2, "f16") == "unsupported"
    assert route_of(33, 264, 8, "f16") == "unsupported" and route_of(33, 264, 2, "f16", aligned=False) == "unsupported"
    assert route_of(33, 264, 2, "u8") == "unsupported" and route_of(33, 260, 2, "i16") == "unsupported"
    # the shapes of test_fp16_frames_through_the_field_warp (the Python layer passes GH = 10 gh)
    for (h, w), gh in (((300, 520), 3), ((200, 264), 2), ((130, 96), 2), ((100, 101), 2)):
        assert route_of(h, w, 10 * gh, "f16") == "unsupported"
    assert route_of(416, 520, 20, "f16") == "warp_field3" and route_of(200, 264, 10, "f16") == "warp_field3"
    tiles = {c: -(-c[1] // TILE_H) * -(-c[2] // TILE_W) for c in FIELD_CASES["warp_field3"]}
    assert any(n % 8 == 0 and n > 8 for n in tiles.values()) and any(n % 8 and n > 8 for n in tiles.values())
    assert 1 in tiles.values()


def _assert_border_caps(lat, h, w, ps, what):
    """h + w on-border pixels per frame with a constant lattice; -> the count of all other frames together."""
    border = coordinate_candidates(lat, h, w, ps)[3].reshape(len(lat), -1).sum(1)
    loose = 0
    for f in range(len(lat)):
        if bool((lat[f] == lat[f, :, :1, :1]).all()):
            assert border[f] <= h + w, (what, f, int(border[f]))
        else:
            loose += int(border[f])
    return loose


def test_cases_reach_every_margin_class_and_stay_off_the_border():
    """From the plan rule (rho = half the range of the nodes a tile touches over ps, n = 3.8 rho + 1.05): the
    tile-frames of EVERY tiled case contain the margins 2, 3, 4, 5, 6 and irregular ones, and a tile that is regular
    for one frame and irregular for another of the same launch -- at ps == 1.0 (the UNIT_PS instantiations of the
    tile kernels and of warp_field_slow) and, separately, at ps != 1.0; every family runs at both kinds of spacing.
    The number of on-border pixels stays under its cap: h + w per frame with a constant lattice, 8 per case for all
    other frames together."""
    for route, case in _all_cases():
        t, h, w, GH, GW = case
        loose = 0
        seen = {True: set(), False: set()}
        mixed = {True: False, False: False}
        families = {True: set(), False: set()}
        for no, ps in case_launches(case):
            unit = ps == 1.0
            lat = case_lattices(case, ps, no)
            families[unit].update((no * t + i) % len(FAMILIES) for i in range(t))
            if not route.startswith("warp_main"):
                mg, _, _ = tile_plan(lat, h, w, ps, field3=route != "warp_field2")
                seen[unit].update(int(v) for v in np.unique(mg))
                irregular = (mg == 0).any(-1)
                mixed[unit] |= bool((irregular.any(0) & ~irregular.all(0)).any())
            loose += _assert_border_caps(lat, h, w, ps, (route, case, no, ps))
        assert loose <= 8, (route, case, loose)
        for unit in (True, False):
            assert families[unit] == set(range(len(FAMILIES))), (route, case, unit)
            if not route.startswith("warp_main"):
                assert seen[unit] >= {0, 2, 3, 4, 5, 6}, (route, case, unit, seen[unit])
                assert mixed[unit], (route, case, unit)
    assert len(FAMILIES) == 12


def test_accumulate_runs_stay_off_the_border_and_split_as_documented():
    """The lattices of test_warp_frames_raw_accumulate_sums_chunks: the same on-border caps, the raw route, no
    irregular tile-frame in the first run and some in the second, at both spacings."""
    assert 1.0 in ACCUM_SPACINGS and any(ps != 1.0 for ps in ACCUM_SPACINGS)
    for kind, case in ACCUM_CASES.items():
        t, h, w, GH, GW = case
        assert route_of(h, w, GH, kind) == "warp_field3"
        for ps in ACCUM_SPACINGS:
            loose = 0
            for run, (families, n) in enumerate(ACCUM_RUNS):
                assert t % n == 0
                lat = accumulate_lattices(case, families, ps)
                irregular = tile_plan(lat, h, w, ps)[0] == 0
                assert bool(irregular.any()) == (run == 1) and not irregular.all()
                loose += _assert_border_caps(lat, h, w, ps, (kind, ps, run))
            assert loose <= 8, (kind, ps, loose)
