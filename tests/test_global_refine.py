"""Iterative sub-pixel whole-frame alignment on the GPU (refine_global_motion, refine_global_motion_raw) against the
float64 restatement (tests/global_refine_reference.py) on the same fp32 movie, with the same number of iterations on
both sides (convergence_threshold = 0, max_iterations = 4).

Shapes: (8, 512, 512) the general K3/K4/K6 route, (6, 1024, 1024) the fused near-window route, (6, 96, 120) the
chirp-z (xcg) route.  The inputs are chosen on the CPU so that every parabola offset of every iteration of the
restatement is at most 0.45 in size: no integer peak can flip between the two sides, and no frame is excluded.

FIELD_TOL: 4 x the worst error measured on an MI355X against the restatement ("Iterative
sub-pixel alignment").
tests/test_refine_chain_float64.py is the judge with a derived bound; the tolerance here stays as a measured guard."""

import numpy as np
import pytest
import torch

import global_refine_reference as gr
from torch_motion_correction_amd import engine

pytestmark = pytest.mark.gpu

SHAPES = [(8, 512, 512), (6, 1024, 1024), (6, 96, 120)]
ITER = 4
FIELD_TOL = 7.6e-6  # px: 4 x 1.9e-6, the worst of the three shapes (field and per-iteration max |r|), one run


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def drifts(t):
    """Planted drifts: whole pixels plus fractions of at most 0.35 px relative to the middle frame (at least 0.3 px
    in one frame: the integer estimate's error)."""
    f = np.arange(t) - t // 2
    dy = np.round(np.linspace(-3, 4, t)) + 0.32 * np.sin(1.3 * f)
    dx = np.round(np.linspace(3, -2, t)) - 0.25 * np.sin(0.9 * f + 0.4) + 0.25 * np.sin(0.4)
    return dy - dy[t // 2], dx - dx[t // 2]


_CASES = {}


def case(shape, noise=0.25):
    """(movie fp32 CPU, texture, truth (t, 2), restatement field (2,t,1,1) float64 after ITER iterations), computed
    once per shape; asserts the condition on the inputs."""
    key = (shape, noise)
    if key not in _CASES:
        t, h, w = shape
        dy, dx = drifts(t)
        movie, tex = gr.planted_movie(t, h, w, dy, dx, noise=noise, seed=h + w)
        want, hist, offs = gr.refine_global_motion(movie, 1.0, max_iterations=ITER, convergence_threshold=0.0,
                                                   return_history=True, return_offsets=True)
        worst = max(float(np.abs(o).max()) for o in offs)
        assert len(offs) == ITER and worst <= 0.45, worst
        _CASES[key] = (movie, tex, np.stack([dy, dx], axis=1), want, hist)
    return _CASES[key]


def field_err(got, want):
    return float((got.detach().cpu().double() - want.double()).abs().max())


@pytest.mark.parametrize("shape", SHAPES)
def test_field_matches_the_restatement(mc, dev, shape):
    movie, _, truth, want, want_hist = case(shape)
    got, hist = mc.refine_global_motion(movie.to(dev), 1.0, max_iterations=ITER, convergence_threshold=0,
                                        return_history=True)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, shape[0], 1, 1) and got.device.type == "cuda"
    assert hist.device.type == "cpu" and tuple(hist.shape) == (ITER,)
    err = field_err(got, want)
    herr = float(np.abs(hist.double().numpy() - np.asarray(want_hist)).max())
    print(f"{shape}: field error {err:.3e} px, history error {herr:.3e} px, max|r| {hist.tolist()}")
    assert err <= FIELD_TOL, err
    assert herr <= FIELD_TOL, herr
    ref = shape[0] // 2
    assert float(got[0, ref, 0, 0]) == 0.0 and float(got[1, ref, 0, 0]) == 0.0


def test_recovers_the_planted_drift_where_the_integer_estimate_cannot(mc, dev):
    movie, _, truth, _, _ = case(SHAPES[0])
    img = movie.to(dev)
    refined = mc.refine_global_motion(img, 1.0, max_iterations=5, convergence_threshold=0)
    integer = mc.estimate_global_motion(img, 1.0)
    as_shifts = lambda f: f[:, :, 0, 0].T.cpu().double().numpy()  # noqa: E731
    err, int_err = np.abs(as_shifts(refined) - truth).max(), np.abs(as_shifts(integer) - truth).max()
    print(f"refined {err:.4f} px, integer {int_err:.4f} px")
    assert err <= 0.1, err
    assert int_err >= 0.3, int_err


def test_pixel_spacing_reference_frame_and_fp16(mc, dev):
    movie, _, _, _, _ = case(SHAPES[0])
    img = movie.to(dev)
    want = gr.refine_global_motion(movie, 1.3, reference_frame=-2, max_iterations=ITER, convergence_threshold=0.0)
    got = mc.refine_global_motion(img, 1.3, reference_frame=-2, max_iterations=ITER, convergence_threshold=0)
    print(f"ps 1.3, reference -2: {field_err(got, want):.3e} A")
    assert field_err(got, want) <= 1.3 * FIELD_TOL, field_err(got, want)
    assert float(got[:, -2].abs().max()) == 0.0
    half = movie.half()
    want16 = gr.refine_global_motion(half.float(), 1.0, max_iterations=ITER, convergence_threshold=0.0)
    got16 = mc.refine_global_motion(half.to(dev), 1.0, max_iterations=ITER, convergence_threshold=0)
    print(f"fp16: {field_err(got16, want16):.3e} px")
    assert field_err(got16, want16) <= FIELD_TOL, field_err(got16, want16)
    # results come back on the caller's device; one frame gives zeros
    cpu = mc.refine_global_motion(movie, 1.0, max_iterations=1, device=None)
    assert cpu.device.type == "cpu"
    one = mc.refine_global_motion(img[:1], 1.0)
    assert tuple(one.shape) == (2, 1, 1, 1) and not one.any()


def test_stops_at_the_threshold(mc, dev):
    movie, _, _, _, _ = case(SHAPES[0])
    field, hist = mc.refine_global_motion(movie.to(dev), 1.0, max_iterations=10, convergence_threshold=0.01,
                                          return_history=True)
    assert 1 <= len(hist) <= 4 and float(hist[-1]) < 0.01 and all(float(x) >= 0.01 for x in hist[:-1]), hist
    assert all(float(b) < float(a) for a, b in zip(hist, hist[1:])), hist


def test_caller_supplied_start_field(mc, dev):
    """A start that is off by (0.4, -0.3) px per frame (alternating in sign, the reference frame included)
    converges to the field of the default start within twice the convergence threshold."""
    movie, _, _, _, _ = case(SHAPES[0])
    img = movie.to(dev)
    thr = 0.01
    base = mc.refine_global_motion(img, 1.0, max_iterations=10, convergence_threshold=thr)
    sign = torch.tensor([(-1.0) ** f for f in range(movie.shape[0])], device=dev)
    start = base.clone()
    start[0, :, 0, 0] += 0.4 * sign
    start[1, :, 0, 0] -= 0.3 * sign
    keep = start.clone()
    got = mc.refine_global_motion(img, 1.0, deformation_field=start, max_iterations=10, convergence_threshold=thr)
    assert torch.equal(start, keep)  # the caller's field is not modified
    assert float((got - base).abs().max()) <= 2 * thr, float((got - base).abs().max())


def central_rms(a, b):
    h, w = a.shape
    box = (slice(h // 4, 3 * h // 4), slice(w // 4, 3 * w // 4))
    return float(((a[box].double() - b[box].double()) ** 2).mean().sqrt())


def test_refined_field_gives_the_sharper_sum(mc, dev):
    """On the low-noise planted movie the Fourier-shift sum is closer to t x the unshifted texture with the refined
    field than with the integer field."""
    movie, tex, _, _, _ = case(SHAPES[0], noise=0.05)
    img = movie.to(dev)
    want = movie.shape[0] * torch.from_numpy(tex)
    refined = mc.refine_global_motion(img, 1.0, max_iterations=5, convergence_threshold=0)
    integer = mc.estimate_global_motion(img, 1.0)
    # the fields are relative to the middle frame, whose planted drift is zero: the sums sit on the texture's grid
    rms_ref = central_rms(mc.motion_correct_sum_fast(img, refined, 1.0).cpu(), want)
    rms_int = central_rms(mc.motion_correct_sum_fast(img, integer, 1.0).cpu(), want)
    print(f"rms refined {rms_ref:.4f}, integer {rms_int:.4f}")
    assert rms_ref < rms_int, (rms_ref, rms_int)


# ------------------------------------------------------------------ raw movies


def range_err(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.max() - b.min()), 1e-30))


def raw_movie(dev, shape, dtype, hot):
    """Detector counts of the planted movie + a gain reference of 1 +- 0.1; with `hot`, a few hot pixels per frame."""
    movie, _, _, _, _ = case(shape)
    t, h, w = shape
    g = torch.Generator().manual_seed(5)
    gain = 1.0 + 0.1 * (2 * torch.rand(h, w, generator=g) - 1)
    if dtype == torch.uint8:
        raw = ((20 * movie + 110) / gain).round().clamp(0, 255).to(dtype)
    else:
        raw = ((300 * movie - 200) / gain).round().clamp(-32768, 32767).to(dtype)
    if hot:
        hi = 255 if dtype == torch.uint8 else 30000
        for f in range(t):
            ys, xs = torch.randint(0, h, (6,), generator=g), torch.randint(0, w, (6,), generator=g)
            raw[f, ys, xs] = hi
            gain[ys, xs] = 1.0
    return raw.to(dev), gain.to(dev)


@pytest.mark.parametrize("hot", [None, 10.0])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
def test_raw_route_matches_the_conditioned_route(mc, dev, dtype, hot, monkeypatch):
    shape = SHAPES[1]
    raw, gain = raw_movie(dev, shape, dtype, hot is not None)
    img = mc.condition_movie(raw, gain, hot_pixel_threshold=hot)
    want = mc.refine_global_motion(img, 1.0, max_iterations=ITER, convergence_threshold=0)

    def refuse(*a, **k):
        raise AssertionError("the fused route conditioned the movie")

    monkeypatch.setattr(engine, "condition_movie", refuse)
    got, hist = mc.refine_global_motion_raw(raw, gain, 1.0, hot_pixel_threshold=hot, max_iterations=ITER,
                                            convergence_threshold=0, return_history=True)
    monkeypatch.undo()
    err = range_err(got, want)
    print(f"{dtype} hot={hot}: raw against conditioned field {err:.3e} of its range")
    assert len(hist) == ITER
    assert err <= 1e-5, err  # the bound of the raw-against-conditioned image tests (tests/test_raw_fast_sums.py)
    assert float(got[:, shape[0] // 2].abs().max()) == 0.0
    # the refined field feeds the existing raw sums: they equal the conditioned route's with the same field
    s_raw = mc.motion_correct_sum_fast_raw(raw, gain, got, 1.0, hot_pixel_threshold=hot)
    s_img = mc.motion_correct_sum_fast(img, got, 1.0)
    if hot is None:
        assert torch.equal(s_raw, s_img)
    else:
        assert range_err(s_raw, s_img) <= 1e-5, range_err(s_raw, s_img)


def test_raw_fallback_is_exactly_the_conditioned_route(mc, dev):
    shape = SHAPES[2]  # no fused raw kernels for 120 columns
    raw, gain = raw_movie(dev, shape, torch.uint8, False)
    got = mc.refine_global_motion_raw(raw, gain, 1.0, max_iterations=ITER, convergence_threshold=0)
    want = mc.refine_global_motion(mc.condition_movie(raw, gain), 1.0, max_iterations=ITER, convergence_threshold=0)
    assert torch.equal(got, want)


def test_existing_estimates_are_untouched(mc, dev):
    """global_shifts_raw keeps its result after the split into spectra + search: bit for bit the integer field."""
    raw, gain = raw_movie(dev, SHAPES[1], torch.uint8, False)
    f1, _ = mc.motion_correct_raw_fast(raw, gain, 1.0)
    f2 = mc.estimate_global_motion(mc.condition_movie(raw, gain), 1.0)
    assert torch.equal(f1, f2)
