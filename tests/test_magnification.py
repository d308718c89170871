"""Magnification distortion correction on the GPU (correct_magnification_distortion -> mc_affine_resample,
csrc/affine_resample.hip) against the float64 restatement of its rule (tests/magnification_reference.py), within the
bound derived there -- cubic_weight_error, the fp32 fraction, fp32 accumulation over 16 taps of magnitude <= max |image|
-- at every pixel, none left out.  Outputs go into NaN-guarded buffers (kernel_harness.nan_buffer): a pixel left
unwritten fails its comparison, a store outside the buffer fails the guard check.  tests/test_magnification_host.py
checks on the CPU that none of these cases puts a source position within 1e-9 of an edge, but for the two columns of
the 1.1 x 1.1 case on 67 columns that sit exactly on it by the rule's unfused arithmetic.

Measured on an MI355X: the worst |kernel - reference| / bound over the general cases is 0.14 (each case prints its
own as a RATIO line)."""

import functools

import numpy as np
import pytest
import torch

import magnification_reference as mr
from kernel_harness import assert_guards, calls, mc, nan_buffer, switches  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda"


def run(mc, image, params, fill_value=0.0, offset=0):
    """The stack (t, h, w) through the module's one route into a guarded buffer -> the (t, h, w) fp32 result on the
    CPU."""
    from torch_motion_correction_amd import magnification

    m = mc.magnification_distortion_matrix(*params)
    src = image.to(DEV).contiguous()
    out, flat = nan_buffer(tuple(src.shape), DEV, offset)
    got = magnification._resample(src, m, float(fill_value), out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert_guards(out, flat, f"mc_affine_resample {tuple(src.shape)} {params}")
    return out.cpu()


@functools.lru_cache(maxsize=None)
def stack(shape):
    return torch.from_numpy(mr.frames(*shape))


@functools.lru_cache(maxsize=None)
def reference(shape, params, fill_value=0.0):
    """(reference float64, bound float64) of the case, computed once and shared."""
    import torch_motion_correction_amd as mc

    m = mc.magnification_distortion_matrix(*params).numpy()
    out, bound = mr.resample(stack(shape).numpy(), m, fill_value)
    out.setflags(write=False)
    bound.setflags(write=False)
    return out, bound


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("shape", [(1, 61, 67), (3, 130, 257)])
def test_identity_returns_the_input_exactly(mc, calls, shape, dtype):
    """Scales of 1: the positions are exact integers, the weights (0, 1, 0, 0), the other taps contribute exact zeros.
    The kernel still runs."""
    img = stack(shape).to(dtype)
    got = run(mc, img, (1.0, 1.0, 0.0), fill_value=9.0, offset=1)
    calls.only("mc_affine_resample", 1)
    assert torch.equal(bits(got), bits(img.float()))
    out = mc.correct_magnification_distortion(img.to(DEV), 1, 1, 77.0)
    assert out.dtype == torch.float32 and out.device.type == "cuda" and torch.equal(bits(out.cpu()), bits(img.float()))


@pytest.mark.parametrize("params", mr.PARAMETERS)
@pytest.mark.parametrize("shape", mr.SHAPES)
def test_general_case_within_the_derived_bound(mc, shape, params):
    want, bound = reference(shape, params)
    got = run(mc, stack(shape), params).double().numpy()
    inside = bound > 0
    assert np.array_equal(got[~inside], want[~inside])  # fill_value 0, exactly, where the reference fills
    err = np.abs(got - want)
    ok = err <= bound  # False for a NaN the kernel left or wrote
    ratio = float((err[inside] / bound[inside]).max())
    print(f"RATIO affine_resample {shape} {params}: {ratio:.3f}")
    assert bool(ok.all()), (f"{int((~ok).sum())} pixels beyond the bound, first {np.argwhere(~ok)[:4].tolist()}, "
                            f"worst |got - want| / bound {ratio:.3f}")
    assert float(np.abs(want - stack(shape).numpy())[inside].max()) > 0.5  # the case resamples


@pytest.mark.parametrize("fill_value", [0.0, -3.5])
def test_filled_pixels_carry_fill_value_bit_for_bit(mc, fill_value):
    shape, params = (3, 130, 257), (1.1, 1.1, 45.0)
    want, bound = reference(shape, params, fill_value)
    got = run(mc, stack(shape), params, fill_value=fill_value)
    fill_bits = int(torch.tensor(fill_value, dtype=torch.float32).view(torch.int32))
    filled = bits(got) == fill_bits
    outside = torch.from_numpy(bound == 0)
    assert int(outside.sum()) == int(filled.sum()) > 0 and torch.equal(filled, outside)
    for y, x in ((0, 0), (0, 256), (129, 0), (129, 256)):
        assert bool(filled[:, y, x].all())
    assert bool((np.abs(got.double().numpy() - want) <= bound).all())


def test_sum_and_one_frame_stack_give_identical_bits(mc):
    img, params = stack((3, 130, 257))[1].to(DEV), (1.02, 0.98, 30.0)
    a = mc.correct_magnification_distortion(img, *params, fill_value=2.0)
    b = mc.correct_magnification_distortion(img[None], *params, fill_value=2.0)
    assert a.shape == (130, 257) and b.shape == (1, 130, 257) and torch.equal(bits(a), bits(b[0]))
    want, bound = reference((3, 130, 257), params, 2.0)
    assert bool((np.abs(a.cpu().double().numpy() - want[1]) <= bound[1]).all())
    # a CPU image comes back on the CPU, `device` says otherwise
    c = mc.correct_magnification_distortion(img.cpu(), *params, fill_value=2.0)
    assert c.device.type == "cpu" and torch.equal(bits(c), bits(a.cpu()))
    assert mc.correct_magnification_distortion(img.cpu(), *params, device=DEV).device.type == "cuda"


def test_two_chunks_give_the_bits_of_one(mc, calls, switches):
    engine, _ = switches
    shape, params = (3, 130, 257), (1.1, 0.9, 117.0)
    one = run(mc, stack(shape), params)
    calls.only("mc_affine_resample", 1)
    calls.clear()
    engine.WORKSPACE_BYTES = 2 * 130 * 257 * 4  # two frames a chunk: 2 + 1
    two = run(mc, stack(shape), params)
    calls.only("mc_affine_resample", 2)
    assert [a[2] for a in calls.args["mc_affine_resample"]] == [2, 1]
    assert torch.equal(bits(one), bits(two))


def test_fp16_equals_the_fp32_result_of_the_upcast_input(mc):
    shape, params = (3, 130, 257), (1.02, 0.98, 30.0)
    half = stack(shape).half()
    a = run(mc, half, params, fill_value=-1.0, offset=3)
    b = run(mc, half.float(), params, fill_value=-1.0)
    assert torch.equal(bits(a), bits(b))
    want, bound = mr.resample(half.float().numpy(), mc.magnification_distortion_matrix(*params).numpy(), -1.0)
    assert bool((np.abs(a.double().numpy() - want) <= bound).all())
