"""Fused Fourier-shift sums of fp32 / fp16 stacks (motion_correct_sum_fast, engine.fast_shift_sums): the plain and
exposure-weighted sums of correct_motion_fast's frames, from one forward transform per frame, against the
composition correct_motion_fast -> .sum(0) / dose_weighted_sum, the oracle, integer shifts and the fallbacks."""

import pytest
import torch

import oracle
from torch_motion_correction_amd import engine

pytestmark = pytest.mark.gpu

REL = 2e-5


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def range_err(a, b):
    """max |a - b| over the range of b"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.max() - b.min()), 1e-30))


def stack(dev, shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * 2.0 + 5.0).to(dev)


def rigid_field(dev, t, amp, seed):
    g = torch.Generator().manual_seed(seed)
    return (amp * (2 * torch.rand(2, t, 1, 1, generator=g) - 1)).to(dev)


def composition(mc, img, field, ps, dose=None, pre=0.0, kv=300.0):
    """The definition: g = field / ps on the device, correct_motion_fast, then the sums."""
    cor = mc.correct_motion_fast(img, field / float(ps))
    plain = cor.sum(0)
    dw = None if dose is None else mc.dose_weighted_sum(cor, ps, dose, pre_exposure=pre, voltage=kv)
    return dw, plain


SHAPES = [((6, 256, 256), 1.0, 1.5, 0.0, 300.0), ((5, 512, 256), 1.3, 0.8, 2.0, 200.0),
          ((3, 256, 1024), 0.83, 2.5, 0.5, 100.0), ((5, 4092, 64), 1.0, 1.2, 0.0, 300.0),
          ((5, 4096, 128), 0.9, 1.1, 0.5, 300.0), ((4, 8184, 128), 0.5, 0.9, 1.0, 300.0),
          ((3, 256, 5760), 1.1, 1.0, 0.0, 200.0), ((2, 4092, 5760), 1.0, 1.3, 0.5, 300.0),
          ((1, 8184, 11520), 0.7, 1.0, 0.0, 300.0)]


@pytest.mark.parametrize("shape,ps,dose,pre,kv", SHAPES)
def test_against_the_composition(mc, dev, shape, ps, dose, pre, kv):
    img = stack(dev, shape, seed=sum(shape))
    field = rigid_field(dev, shape[0], 6.0 * ps, seed=shape[1])
    keep = field.clone()
    want_dw, want_plain = composition(mc, img, field, ps, dose, pre, kv)
    plain = mc.motion_correct_sum_fast(img, field, ps)
    dw, plain2 = mc.motion_correct_sum_fast(img, field, ps, dose_per_frame=dose, pre_exposure=pre, voltage=kv,
                                            return_plain_sum=True)
    dw_only = mc.motion_correct_sum_fast(img, field, ps, dose_per_frame=dose, pre_exposure=pre, voltage=kv)
    assert torch.equal(field, keep)  # the caller's grid is never negated
    assert range_err(plain, want_plain) <= REL, range_err(plain, want_plain)
    assert range_err(dw, want_dw) <= REL, range_err(dw, want_dw)
    assert torch.equal(plain2, plain)  # the plain sum does not depend on the dose being accumulated alongside
    assert torch.equal(dw_only, dw)


def test_many_chunks_40_frames_of_4096(mc, dev):
    t, h, w = 40, 4096, 4096
    img = stack(dev, (t, h, w), seed=40)
    field = rigid_field(dev, t, 12.0, seed=41)
    assert engine.WORKSPACE_BYTES // (2 * h * 2064 * 8) < t  # more than one chunk of frames
    want_dw, want_plain = composition(mc, img, field, 1.0, 1.0, 0.5, 300.0)
    dw, plain = mc.motion_correct_sum_fast(img, field, 1.0, dose_per_frame=1.0, pre_exposure=0.5,
                                           return_plain_sum=True)
    assert range_err(plain, want_plain) <= REL, range_err(plain, want_plain)
    assert range_err(dw, want_dw) <= REL, range_err(dw, want_dw)


@pytest.mark.parametrize("shape,ps,dose", [((6, 256, 256), 1.0, 1.5), ((5, 512, 256), 1.3, 0.8),
                                           ((3, 256, 1024), 0.83, 2.5)])
def test_against_the_oracle(mc, dev, shape, ps, dose):
    img = stack(dev, shape, seed=7 + shape[0])
    field = rigid_field(dev, shape[0], 5.0 * ps, seed=8)
    dw, plain = mc.motion_correct_sum_fast(img, field, ps, dose_per_frame=dose, return_plain_sum=True)
    g = field.cpu() / ps
    cor = oracle.correct_motion_fast(img.cpu(), g)
    ref_plain = cor.sum(0)
    ref_dw = oracle.dose_weighted_sum(cor, ps, dose)
    assert float((plain.cpu() - ref_plain).abs().max()) <= 1e-4 * float(ref_plain.abs().max())
    assert float((dw.cpu() - ref_dw).abs().max()) <= 1e-4 * float(ref_dw.abs().max())


@pytest.mark.parametrize("shape", [(4, 256, 512), (3, 4096, 256), (3, 4092, 128)])
def test_integer_shifts_are_rolls(mc, dev, shape):
    t = shape[0]
    img = stack(dev, shape, seed=3)
    sh = torch.tensor([[3.0 + f, -7.0 + 2 * f] for f in range(t)])  # (t, 2) px
    field = sh.t()[:, :, None, None].contiguous().to(dev)  # shifted by -field, as correct_motion_fast
    got = mc.motion_correct_sum_fast(img, field, 1.0).cpu().double()
    want = sum(torch.roll(img[f].cpu().double(), shifts=(-int(sh[f, 0]), -int(sh[f, 1])), dims=(0, 1))
               for f in range(t))
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-5


def test_fp16_stack_is_its_fp32_copy(mc, dev):
    img = stack(dev, (4, 512, 512), seed=5).half()
    field = rigid_field(dev, 4, 3.0, seed=6)
    got = mc.motion_correct_sum_fast(img, field, 1.0, dose_per_frame=1.0, return_plain_sum=True)
    want = mc.motion_correct_sum_fast(img.float(), field, 1.0, dose_per_frame=1.0, return_plain_sum=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("case", ["example_frames", "chirp_z_width", "polyphase"])
def test_fallbacks_are_exactly_the_composition(mc, dev, case, monkeypatch):
    shape = {"example_frames": (3, 959, 927), "chirp_z_width": (3, 256, 600), "polyphase": (3, 256, 512)}[case]
    if case == "polyphase":
        monkeypatch.setattr(engine, "POLYPHASE_FOURIER_SHIFT", True)
    else:
        assert not engine._full_row_major_ok(*shape[1:])
    img = stack(dev, shape, seed=11)
    field = rigid_field(dev, shape[0], 4.0, seed=12)
    want_dw, want_plain = composition(mc, img, field, 1.2, 1.1, 0.3, 300.0)
    dw, plain = mc.motion_correct_sum_fast(img, field, 1.2, dose_per_frame=1.1, pre_exposure=0.3,
                                           return_plain_sum=True)
    assert torch.equal(dw, want_dw) and torch.equal(plain, want_plain)
    assert torch.equal(mc.motion_correct_sum_fast(img, field, 1.2), want_plain)


def test_cpu_inputs_come_back_on_the_cpu(mc, dev):
    img = stack(dev, (3, 256, 256), seed=2)
    field = rigid_field(dev, 3, 2.0, seed=2)
    got = mc.motion_correct_sum_fast(img.cpu(), field.cpu(), 1.0)
    assert got.device.type == "cpu"
    assert torch.equal(got, mc.motion_correct_sum_fast(img, field, 1.0).cpu())
