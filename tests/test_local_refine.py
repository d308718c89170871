"""Iterative sub-pixel patch alignment on the GPU (refine_local_motion) against the float64 restatement
(tests/local_refine_reference.py) on the same fp32 movie, with the same number of iterations on both sides
(convergence_threshold = 0, max_iterations = 4) and pixel spacing 1.

Shapes: (6, 1536, 2048) with 1024-px patches (the wave-per-row patch engine and the fused near-window search),
(8, 512, 640) with 256-px patches (the workgroup engine), (6, 200, 240) with 96-px patches (the chirp-z route).  The
movies carry planted LOCAL motion (local_refine_reference.planted_local_movie).  The case builder asserts on the CPU,
for every patch of every frame and every iteration of the restatement, that the parabola offsets are at most 0.45 in
size and the residuals lie inside (-15, +47) px: no integer peak can flip between the two sides, no residual leaves
the near window, and no patch is left out.

FIELD_TOL: the whole-frame route's 7.6e-6 px (tests/test_global_refine.py: 4 x 1.9e-6 px).  The patch route's own worst
error, measured on an MI355X in one run of this file, is 3.6e-6 px (field 2.8e-6, per-iteration max |r| 3.6e-6; DESIGN
section 4, "Iterative patch alignment"); 4 x that is 1.4e-5 px, larger than today's value, so FIELD_TOL stays where it
is.  Above 1e-4 px is a bug, not a tolerance.  tests/test_refine_chain_float64.py is the judge with a derived bound."""

import numpy as np
import pytest
import torch

import local_refine_reference as lr

pytestmark = pytest.mark.gpu

CASES = [((6, 1536, 2048), 1024), ((8, 512, 640), 256), ((6, 200, 240), 96)]
ITER = 4
FIELD_TOL = 7.6e-6  # px: the whole-frame route's 4 x 1.9e-6; 4 x the patch route's own 3.6e-6 would be larger (see above)


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def drifts(t, big=0.0):
    """Planted motion relative to the middle frame: the rigid part is whole pixels plus a fraction of at most 0.2 px
    (`big`: plus an alternating whole-pixel drift of that size), the local part changes by up to 0.45 px (y) and
    0.6 px (x) from the left to the right edge of the frame."""
    f = np.arange(t) - t // 2
    ay = np.round(np.linspace(-3, 4, t)) + 0.2 * np.sin(1.3 * f) + big * (f % 2) * np.sign(f)
    ax = np.round(np.linspace(3, -2, t)) - 0.15 * np.sin(0.9 * f + 0.4) + 0.15 * np.sin(0.4) - big * (f % 2)
    rigid = np.stack([ay - ay[t // 2], ax - ax[t // 2]], axis=1)
    slope = np.stack([0.45 * np.sin(0.8 * f), -0.6 * f / (t // 2)], axis=1)
    return rigid, slope


def integer_field(rigid):
    """The rigid part rounded to whole pixels as a (2, t, 1, 1) field (pixel spacing 1): the start of the cases."""
    return torch.from_numpy(np.rint(rigid)).float().T[:, :, None, None].contiguous()


_CASES = {}


def case(shape, p, big=0.0, half=False, pixel_spacing=1.0, reference_frame=None, noise=0.25):
    """(movie fp32 CPU, start field in Angstrom, truth (t, npatch, 2) px, restatement field (2, t, gh, gw) float64
    after ITER iterations, its history), computed once per key; asserts the conditions on the inputs for ALL
    patches.  `half`: the movie rounded to fp16 values."""
    key = (shape, p, big, half, pixel_spacing, reference_frame, noise)
    if key not in _CASES:
        t, h, w = shape
        rigid, slope = drifts(t, big)
        movie, drift = lr.planted_local_movie(t, h, w, rigid, slope, noise=noise, seed=h + w)
        if half:
            movie = movie.half().float()
        ref = t // 2 if reference_frame is None else reference_frame % t
        start = integer_field(rigid - rigid[ref]) * pixel_spacing
        want, info = lr.refine_local_motion(movie, pixel_spacing, p, start, reference_frame, max_iterations=ITER,
                                            convergence_threshold=0.0, details=True)
        check_conditions(info)
        _CASES[key] = (movie, start, lr.planted_truth(drift, shape, p, reference_frame), want, info["history"])
    return _CASES[key]


def check_conditions(info):
    assert len(info["parabola"]) == ITER
    worst = max(float(np.abs(o).max()) for o in info["parabola"])
    lo = min(float(r.min()) for r in info["residuals"])
    hi = max(float(r.max()) for r in info["residuals"])
    assert worst <= 0.45, worst
    assert -15 < lo and hi < 47, (lo, hi)


def field_err(got, want):
    return float((got.detach().cpu().double() - want.double()).abs().max())


def hist_err(hist, want_hist):
    return float(np.abs(hist.double().numpy() - np.asarray(want_hist)).max())


@pytest.mark.parametrize("shape,p", CASES)
def test_field_matches_the_restatement(mc, dev, shape, p):
    movie, start, _, want, want_hist = case(shape, p)
    got, centres, hist = mc.refine_local_motion(movie.to(dev), 1.0, p, deformation_field=start.to(dev),
                                                max_iterations=ITER, convergence_threshold=0, return_history=True)
    t = shape[0]
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) and got.device.type == "cuda"
    assert hist.device.type == "cpu" and tuple(hist.shape) == (ITER,)
    err, herr = field_err(got, want), hist_err(hist, want_hist)
    print(f"{shape} p={p}: field error {err:.3e} px, history error {herr:.3e} px, max|r| {hist.tolist()}")
    assert err <= FIELD_TOL, err
    assert herr <= FIELD_TOL, herr
    assert float(got[:, t // 2].abs().max()) == 0.0
    assert float(got.abs().max()) > 1.0
    # the lattice is the patch estimator's
    _, want_centres = mc.estimate_motion_cross_correlation_patches(movie.to(dev), 1.0, patch_sidelength=p)
    assert centres.dtype == torch.int64 and torch.equal(centres, want_centres)


def test_large_start_moves_the_windows_and_clamps_at_the_edges(mc, dev):
    """A +-12 px alternating drift, planted and given as the start: the windows are cut 12 px off the lattice, and
    those of the border patches are clamped to the frame, on both sides by the same rule."""
    shape, p = CASES[1]
    movie, start, _, want, want_hist = case(shape, p, big=12.0)
    o = lr.window_offsets(lr.start_px(start, 1.0, shape, p), shape, p)
    assert np.abs(o).max() >= 12 and (np.abs(o) < 12).any() and (np.abs(o).max(axis=(1, 2)) >= 12).sum() >= 4
    got, _, hist = mc.refine_local_motion(movie.to(dev), 1.0, p, deformation_field=start.to(dev), max_iterations=ITER,
                                          convergence_threshold=0, return_history=True)
    err, herr = field_err(got, want), hist_err(hist, want_hist)
    print(f"+-12 px start: field error {err:.3e} px, history error {herr:.3e} px, max|r| {hist.tolist()}")
    assert err <= FIELD_TOL and herr <= FIELD_TOL, (err, herr)
    assert float(got[:, shape[0] // 2].abs().max()) == 0.0


def test_pixel_spacing_and_reference_frame(mc, dev):
    shape, p = CASES[1]
    movie, start, _, want, want_hist = case(shape, p, pixel_spacing=1.3, reference_frame=-2)
    got, _, hist = mc.refine_local_motion(movie.to(dev), 1.3, p, deformation_field=start.to(dev), reference_frame=-2,
                                          max_iterations=ITER, convergence_threshold=0, return_history=True)
    err = field_err(got, want)
    print(f"ps 1.3, reference -2: {err:.3e} A, history {hist_err(hist, want_hist):.3e} px")
    assert err <= 1.3 * FIELD_TOL, err
    assert hist_err(hist, want_hist) <= FIELD_TOL
    assert float(got[:, -2].abs().max()) == 0.0 and float(got[:, shape[0] // 2].abs().max()) > 0.0


def test_fp16_stack_device_of_the_result_and_one_frame(mc, dev):
    shape, p = CASES[0]
    movie, start, _, want, want_hist = case(shape, p, half=True)
    got, _, hist = mc.refine_local_motion(movie.half().to(dev), 1.0, p, deformation_field=start.to(dev),
                                          max_iterations=ITER, convergence_threshold=0, return_history=True)
    err = field_err(got, want)
    print(f"fp16: {err:.3e} px, history {hist_err(hist, want_hist):.3e} px")
    assert err <= FIELD_TOL and hist_err(hist, want_hist) <= FIELD_TOL, err
    # results come back on the caller's device; one frame gives zeros
    small, sp = CASES[2]
    cpu_field, cpu_centres = mc.refine_local_motion(case(small, sp)[0], 1.0, sp, max_iterations=1)
    assert cpu_field.device.type == "cpu" and cpu_centres.device.type == "cpu"
    one, c1 = mc.refine_local_motion(case(small, sp)[0][:1].to(dev), 1.0, sp)
    assert tuple(one.shape) == (2, 1, 3, 3) and not one.any() and tuple(c1.shape) == (1, 3, 3, 3)


def test_default_start_is_the_refined_global_field(mc, dev):
    """deformation_field=None starts from refine_global_motion on the same movie -- on both sides."""
    shape, p = CASES[2]
    movie = case(shape, p)[0]
    want, info = lr.refine_local_motion(movie, 1.0, p, max_iterations=ITER, convergence_threshold=0.0, details=True)
    check_conditions(info)
    img = movie.to(dev)
    got, _, hist = mc.refine_local_motion(img, 1.0, p, max_iterations=ITER, convergence_threshold=0,
                                          return_history=True)
    err, herr = field_err(got, want), hist_err(hist, info["history"])
    print(f"default start: field error {err:.3e} px, history error {herr:.3e} px")
    assert err <= FIELD_TOL and herr <= FIELD_TOL, (err, herr)
    same = mc.refine_local_motion(img, 1.0, p, deformation_field=mc.refine_global_motion(img, 1.0), max_iterations=ITER,
                                  convergence_threshold=0)[0]
    assert torch.equal(same, got)


def test_stops_at_the_threshold(mc, dev):
    shape, p = CASES[1]
    movie, start, _, _, _ = case(shape, p)
    _, _, hist = mc.refine_local_motion(movie.to(dev), 1.0, p, deformation_field=start, max_iterations=10,
                                        convergence_threshold=0.01, return_history=True)
    assert 1 <= len(hist) < 10 and float(hist[-1]) < 0.01 and all(float(x) >= 0.01 for x in hist[:-1]), hist


def test_recovers_planted_local_motion_where_the_rigid_field_cannot(mc, dev):
    """A local part of 0.8 px (y) and 2 px (x) across the frame: +-0.5 px at the centres of the two 1024-px patches."""
    shape, p = CASES[0]
    t = shape[0]
    f = np.arange(t) - t // 2
    rigid = np.stack([np.linspace(-3.3, 4.6, t), np.linspace(2.7, -1.9, t)], axis=1)
    slope = np.stack([0.8 * np.sin(0.8 * f), -2.0 * f / (t // 2)], axis=1)
    movie, drift = lr.planted_local_movie(*shape, rigid, slope, noise=0.25, seed=9)
    truth = lr.planted_truth(drift, shape, p)
    img = movie.to(dev)
    rigid_field = mc.refine_global_motion(img, 1.0)
    field, _ = mc.refine_local_motion(img, 1.0, p, max_iterations=5, convergence_threshold=0)
    as_shifts = lambda f: f.permute(1, 2, 3, 0).reshape(t, -1, 2).cpu().double().numpy()  # noqa: E731
    err = np.abs(as_shifts(field) - truth).max()
    rigid_err = np.abs(as_shifts(rigid_field.expand(2, t, *field.shape[2:])) - truth).max()
    print(f"refined {err:.4f} px, rigid start {rigid_err:.4f} px")
    assert err <= 0.1, err
    assert rigid_err >= 0.3, rigid_err
