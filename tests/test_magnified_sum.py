"""The aligned sum with the magnification map folded into the rigid warp on the GPU (motion_correct_sum_magnified,
motion_correct_sum_magnified_raw -> mc_affine_warp_sum, csrc/affine_warp_sum.hip) against the float64 restatement of
its rule (tests/magnified_sum_reference.py), within the bound derived there -- the resampler's bound per frame over the
pixel's own taps, plus the fp32 sequential sum's roundings -- at every pixel, none left out; and bit for bit against
what the rule says must be equal: the exact whole-pixel sums under identity M, the stand-alone resampler at a zero
field, the frames against the sum, fp16 against its up-cast, the raw kinds against the conditioned movie.  Outputs go
into NaN-guarded buffers (kernel_harness.nan_buffer): a pixel left unwritten fails its comparison, a store outside the
buffer fails the guard check.

Measured on an MI355X: the worst |kernel - reference| / bound over the general cases is 0.16 (each case prints its
own as a RATIO line)."""

import functools

import numpy as np
import pytest
import torch

import magnification_reference as mr
import magnified_sum_reference as ms
import rigid_reference as rr
from kernel_harness import assert_guards, calls, mc, nan_buffer, raw_movie  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
GENERAL = ((3, 130, 257), (1.02, 0.98, 30.0), 0.83)  # the general case of the bit-for-bit tests: shape, parameters, ps


def bits(t):
    return t.contiguous().view(torch.int32)


def field_of(shifts_px, ps):
    """Whole-pixel node shifts (t, 2) -> the (2, t, 1, 1) fp32 Angstrom field fp32(s * ps) of a catmull_rom field."""
    s = np.asarray(shifts_px, dtype=F32)
    return torch.from_numpy((s * F32(ps)).astype(F32).T.copy()[:, :, None, None])


def run(mc, src, field, ps, params, gain=None, mean_zero=False, want_frames=False, offset=0):
    """The (t, h, w) movie `src` (fp32 / fp16: the float route; u8 / i16 with `gain`: the raw route, one
    engine.RawMovie) through mc_affine_warp_sum into guarded buffers -> (sum (h, w), frames (t, h, w) or None) on the
    CPU."""
    from torch_motion_correction_amd import engine, magnification

    t, h, w = src.shape
    shifts = magnification._pixel_shifts(field, t, ps)
    matrix = mc.magnification_distortion_matrix(*params)
    dev_src = src.to(DEV).contiguous()
    total, total_flat = nan_buffer((h, w), DEV, offset)
    frames, frames_flat = nan_buffer((t, h, w), DEV, offset) if want_frames else (None, None)
    if src.dtype in (torch.uint8, torch.int16):
        rm = engine.RawMovie(dev_src, None if gain is None else gain.to(DEV), mean_zero=mean_zero)
        args = (rm.raw, rm.kind, rm.gain, rm.mu)
    else:
        args = (dev_src, engine.storage_of(dev_src), None, None)
    got = magnification._warp_sum(*args, matrix, shifts, want_frames, out=(total, frames))
    torch.cuda.synchronize()
    assert got[0].data_ptr() == total.data_ptr()
    what = f"mc_affine_warp_sum {tuple(src.shape)} {src.dtype} {params}"
    assert_guards(total, total_flat, what)
    if want_frames:
        assert_guards(frames, frames_flat, what + " frames")
    return total.cpu(), frames.cpu() if want_frames else None


@functools.lru_cache(maxsize=None)
def stack(shape):
    return torch.from_numpy(mr.frames(*shape))


@functools.lru_cache(maxsize=None)
def reference(shape, params, ps):
    """(field (2, t, 1, 1) fp32 tensor, sum float64, bound float64) of a general case, computed once and shared."""
    import torch_motion_correction_amd as mc

    # |shift| up to 20 px, but no further than half the frame: a 4 x 4 frame would otherwise be sampled nowhere
    max_shift = min(ms.MAX_SHIFT, (min(shape[1:]) - 1) / 2)
    field = ms.case_field(shape[0], ps, max_shift=max_shift)
    shifts = ms.pixel_shifts(field, ps)
    assert 0.25 * max_shift < np.abs(shifts).max() <= max_shift + 1e-3 and (shifts != np.round(shifts)).all()
    m = mc.magnification_distortion_matrix(*params).numpy()
    total, bound, _, _, ins = ms.magnified_sum(stack(shape).numpy(), m, shifts)
    total.setflags(write=False)
    bound.setflags(write=False)
    return torch.from_numpy(field), total, bound, ins.any(0)


# ------------------------------------------------------------------ 1: identity M, whole-pixel shifts: exact


WHOLE = {(3, 130, 257): ((-3, 5), (6, -13), (0, -3)),      # -3 px: at ps = 0.83 the reciprocal rounding drops row 3
         (5, 64, 64): ((-3, 3), (15, -6), (0, 0), (-9, 62), (7, -70))}  # the last frame: wholly outside


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.uint8, torch.int16])
@pytest.mark.parametrize("ps", [1.0, 0.83])
@pytest.mark.parametrize("shape", sorted(WHOLE))
def test_identity_and_whole_pixel_shifts_give_the_exact_sequential_sum(mc, calls, shape, ps, dtype):
    t, h, w = shape
    shifts = np.array(WHOLE[shape], dtype=F32)
    field = field_of(shifts, ps)
    assert np.array_equal(ms.pixel_shifts(field.numpy(), ps), shifts)  # the canonical quotient returns the node shifts
    if ps == 0.83:
        assert -3 in rr.row_dropping_shifts(shifts[:, 0], ps)
    gain = None
    if dtype in (torch.uint8, torch.int16):
        src = raw_movie(t, h, w, dtype, seed=21)
        assert dtype == torch.uint8 or bool((src < 0).any())
        gain = torch.randint(0, 4, (h, w), generator=torch.Generator().manual_seed(4)).float()  # whole numbers: exact
        values = src.float() * gain
    else:
        src = stack(shape).to(dtype)
        values = src.float()
    got, _ = run(mc, src, field, ps, (1.0, 1.0, 0.0), gain=gain, mean_zero=False, offset=1)
    calls.ran("mc_affine_warp_sum")
    assert calls.count("mc_affine_warp_sum") == 1
    want = ms.sequential_sum(ms.shifted_zero_outside(values.numpy(), shifts))
    assert torch.equal(bits(got), bits(torch.from_numpy(want)))
    assert bool((got[3] != 0).any())  # output row 3 samples row 0 of the first frame: kept


# ------------------------------------------------------------------ 2: zero field, one frame: the stand-alone resampler


@pytest.mark.parametrize("params", mr.PARAMETERS)
@pytest.mark.parametrize("shape", [(1, 61, 67), (1, 130, 257)])
def test_zero_field_one_frame_equals_the_resampler_bit_for_bit(mc, calls, shape, params):
    img = stack((3, 130, 257))[1:2] if shape == (1, 130, 257) else stack(shape)
    got, _ = run(mc, img, torch.zeros(2, 1, 1, 1), 0.83, params)
    calls.only("mc_affine_warp_sum", 1)
    want = mc.correct_magnification_distortion(img[0].to(DEV), *params, fill_value=0.0).cpu()
    assert torch.equal(bits(got), bits(want))
    assert bool((got != img[0]).any())


# ------------------------------------------------------------------ 3: the general case within the derived bound


@pytest.mark.parametrize("params", ms.PARAMETERS)
@pytest.mark.parametrize("shape", ms.SHAPES)
def test_general_case_within_the_derived_bound(mc, calls, shape, params):
    ps = 0.83
    field, want, bound, sampled = reference(shape, params, ps)
    got, _ = run(mc, stack(shape), field, ps, params, offset=2)
    calls.only("mc_affine_warp_sum", 1)
    got = got.double().numpy()
    assert np.array_equal(got[bound == 0], want[bound == 0])  # exactly 0 where no frame contributes
    err = np.abs(got - want)
    ok = err <= bound  # False for a NaN the kernel left or wrote
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"RATIO magnified_sum {shape} {params}: {ratio:.3f}")
    assert bool(ok.all()), (f"{int((~ok).sum())} pixels beyond the bound, first {np.argwhere(~ok)[:4].tolist()}, "
                            f"worst |got - want| / bound {ratio:.3f}")
    assert bool(sampled.any()) and np.array_equal(bound > 0, sampled)
    plain = stack(shape).numpy().astype(np.float64).sum(0)
    assert float(np.abs(want - plain)[sampled].max()) > (0.5 if shape[1] * shape[2] > 16 else 0.0)  # the case resamples


# ------------------------------------------------------------------ 4: the frames against the sum


def test_frames_sum_to_the_sum_and_equal_one_frame_movies(mc, calls):
    shape, params, ps = GENERAL
    field = reference(shape, params, ps)[0]
    total, _ = run(mc, stack(shape), field, ps, params)
    both, frames = run(mc, stack(shape), field, ps, params, want_frames=True, offset=3)
    assert calls.names == ["mc_affine_warp_sum"] * 2
    assert calls.args["mc_affine_warp_sum"][0][10] is None and calls.args["mc_affine_warp_sum"][1][10] is not None
    assert torch.equal(bits(total), bits(both))
    for f in range(shape[0]):
        one, _ = run(mc, stack(shape)[f:f + 1], field[:, f:f + 1], ps, params)
        assert torch.equal(bits(frames[f]), bits(one)), f
    assert torch.equal(bits(torch.from_numpy(ms.sequential_sum(frames.numpy()))), bits(total))
    # the public call returns the same pair
    s, fr = mc.motion_correct_sum_magnified(stack(shape).to(DEV), field, ps, *params, return_frames=True)
    assert s.device.type == "cuda" and fr.shape == shape and fr.dtype == torch.float32
    assert torch.equal(bits(s.cpu()), bits(total)) and torch.equal(bits(fr.cpu()), bits(frames))


# ------------------------------------------------------------------ 5: fp16


def test_fp16_equals_the_fp32_result_of_the_upcast_input(mc, calls):
    shape, params, ps = GENERAL
    field = reference(shape, params, ps)[0]
    half = stack(shape).half()
    a, fa = run(mc, half, field, ps, params, want_frames=True, offset=1)
    b, fb = run(mc, half.float(), field, ps, params, want_frames=True)
    calls.only("mc_affine_warp_sum", 2)
    assert [c[1] for c in calls.args["mc_affine_warp_sum"]] == [2, 3]  # MC_STORE_F16, MC_STORE_F32
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(fa), bits(fb))


# ------------------------------------------------------------------ 6: raw movies against the conditioned movie


def zero_gain(h, w):
    """A random fp32 gain in [0.5, 1.5) with a few exact zeros (dead pixels)."""
    g = torch.Generator().manual_seed(h * 13 + w)
    gain = torch.rand(h, w, generator=g) + 0.5
    gain.view(-1)[torch.randperm(h * w, generator=g)[:9]] = 0.0
    return gain


# (5, 64, 64) with and without the mean: mc_raw_movie_stats and mc_condition_movie sum such a frame (w % 8 == 0) in one
# order, so the means agree in every bit; the odd shape without the mean, where mu = 0 on both sides
@pytest.mark.parametrize("shape,mean_zero", [((5, 64, 64), True), ((5, 64, 64), False), ((3, 130, 257), False)])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
def test_raw_movie_equals_the_conditioned_route_bit_for_bit(mc, calls, dtype, shape, mean_zero):
    t, h, w = shape
    params, ps = GENERAL[1], GENERAL[2]
    field = reference(shape, params, ps)[0]
    movie, gain = raw_movie(t, h, w, dtype, seed=33), zero_gain(h, w)
    assert dtype == torch.uint8 or bool((movie < 0).any())
    got, frames = run(mc, movie, field, ps, params, gain=gain, mean_zero=mean_zero, want_frames=True, offset=1)
    calls.ran("mc_raw_movie_stats", "mc_affine_warp_sum", absent=("mc_condition_movie",))
    assert calls.args["mc_affine_warp_sum"][0][1] == (0 if dtype == torch.uint8 else 1)
    conditioned = mc.condition_movie(movie.to(DEV), gain.to(DEV), mean_zero=mean_zero)
    want, want_frames = mc.motion_correct_sum_magnified(conditioned, field, ps, *params, return_frames=True)
    assert torch.equal(bits(got), bits(want.cpu())) and torch.equal(bits(frames), bits(want_frames.cpu()))
    # the public raw call gives the same, and the result is within the bound of the conditioned movie's restatement
    pub = mc.motion_correct_sum_magnified_raw(movie.to(DEV), gain, field, ps, *params, mean_zero=mean_zero)
    assert torch.equal(bits(pub.cpu()), bits(got))
    m = mc.magnification_distortion_matrix(*params).numpy()
    ref, bound, _, _, _ = ms.magnified_sum(conditioned.cpu().numpy(), m, ms.pixel_shifts(field.numpy(), ps))
    assert bool((np.abs(got.double().numpy() - ref) <= bound).all())
    if mean_zero:
        assert abs(float(conditioned.mean())) < 1e-3 < float(conditioned.abs().mean())


def test_raw_movie_without_a_gain_takes_ones(mc):
    shape, params, ps = (5, 64, 64), GENERAL[1], GENERAL[2]
    field = reference(shape, params, ps)[0]
    movie = raw_movie(*shape, torch.uint8, seed=34).to(DEV)
    a = mc.motion_correct_sum_magnified_raw(movie, None, field, ps, *params)
    b = mc.motion_correct_sum_magnified_raw(movie, torch.ones(64, 64), field, ps, *params)
    assert torch.equal(bits(a.cpu()), bits(b.cpu()))


# ------------------------------------------------------------------ 7: a frame shifted wholly outside


def test_a_frame_shifted_wholly_outside_contributes_nothing(mc, calls):
    shape, params, ps = GENERAL
    field = reference(shape, params, ps)[0].clone()
    field[:, 1, 0, 0] = torch.tensor([400.0 * ps, -700.0 * ps])  # beyond the 130 x 257 frame on both axes
    got, frames = run(mc, stack(shape), field, ps, params, want_frames=True)
    keep = [0, 2]
    want, _ = run(mc, stack(shape)[keep], field[:, keep], ps, params)
    calls.only("mc_affine_warp_sum", 2)
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(frames[1]), torch.zeros(shape[1:], dtype=torch.int32))  # +0.0 everywhere
    assert bool((frames[0] != 0).any()) and bool((frames[2] != 0).any())


# ------------------------------------------------------------------ 8: CPU input, device=


def test_cpu_input_comes_back_on_the_cpu_and_device_is_honoured(mc):
    shape, params, ps = GENERAL
    field = reference(shape, params, ps)[0]
    on_gpu = mc.motion_correct_sum_magnified(stack(shape).to(DEV), field, ps, *params)
    assert on_gpu.device.type == "cuda" and on_gpu.dtype == torch.float32 and on_gpu.shape == shape[1:]
    on_cpu = mc.motion_correct_sum_magnified(stack(shape), field, ps, *params)
    assert on_cpu.device.type == "cpu" and torch.equal(bits(on_cpu), bits(on_gpu.cpu()))
    moved = mc.motion_correct_sum_magnified(stack(shape), field.to(DEV), ps, *params, device=DEV)
    assert moved.device.type == "cuda" and torch.equal(bits(moved.cpu()), bits(on_cpu))
    back, fr = mc.motion_correct_sum_magnified(stack(shape).to(DEV), field, ps, *params, return_frames=True, device="cpu")
    assert back.device.type == "cpu" and fr.device.type == "cpu" and torch.equal(bits(back), bits(on_cpu))
    movie, gain = raw_movie(*shape, torch.int16, seed=35), zero_gain(*shape[1:])
    raw_cpu = mc.motion_correct_sum_magnified_raw(movie, gain, field, ps, *params, mean_zero=False)
    raw_gpu = mc.motion_correct_sum_magnified_raw(movie, gain, field, ps, *params, mean_zero=False, device=DEV)
    assert raw_cpu.device.type == "cpu" and raw_gpu.device.type == "cuda" and torch.equal(bits(raw_cpu), bits(raw_gpu.cpu()))
