"""Host-side checks of the dose-weighted sums from raw movies (motion_correct_sum_raw, motion_correct_raw's dose
keywords, mc_warp_rigid_raw_accumulate / mc_warp_frames_raw_accumulate): the public signatures, argument validation
before any device is touched, and the C entry points' own checks (no launch)."""

import ctypes
import inspect

import pytest
import torch

from kernel_harness import assert_entry_point
from torch_motion_correction_amd import _lib

U8, I16 = 0, 1


def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def test_public_entry_point_and_defaults():
    import torch_motion_correction_amd as mc

    assert "motion_correct_sum_raw" in mc.__all__
    sig = inspect.signature(mc.motion_correct_sum_raw)
    assert list(sig.parameters)[:4] == ["movie", "gain", "deformation_grid", "pixel_spacing"]
    assert _defaults(mc.motion_correct_sum_raw) == dict(
        grid_type="catmull_rom", mean_zero=True, hot_pixel_threshold=None, dose_per_frame=None, pre_exposure=0.0,
        voltage=300.0, return_plain_sum=False, return_frames=False, device=None)


def test_motion_correct_raw_gains_the_dose_keywords_at_the_end():
    import torch_motion_correction_amd as mc

    names = list(inspect.signature(mc.motion_correct_raw).parameters)
    assert names[-3:] == ["dose_per_frame", "pre_exposure", "voltage"]
    assert names[:-3] == ["movie", "gain", "pixel_spacing", "reference_frame", "b_factor", "frequency_range",
                          "grid_type", "mean_zero", "return_frames", "device", "hot_pixel_threshold",
                          "return_hot_counts"]
    d = _defaults(mc.motion_correct_raw)
    assert (d["dose_per_frame"], d["pre_exposure"], d["voltage"]) == (None, 0.0, 300.0)


def _raw_and_field(t=3, h=64, w=64, gh=1, gw=1):
    return torch.zeros((t, h, w), dtype=torch.uint8), torch.zeros((2, t, gh, gw))


@pytest.mark.parametrize("kw,match", [(dict(dose_per_frame=-0.1), "dose_per_frame"),
                                      (dict(dose_per_frame=float("nan")), "dose_per_frame"),
                                      (dict(dose_per_frame=float("inf")), "dose_per_frame"),
                                      (dict(dose_per_frame="one"), "dose_per_frame"),
                                      (dict(return_plain_sum=True), "return_plain_sum"),
                                      (dict(hot_pixel_threshold=0.0), "hot_pixel_threshold"),
                                      (dict(hot_pixel_threshold=float("nan")), "hot_pixel_threshold"),
                                      (dict(hot_pixel_threshold="ten"), "hot_pixel_threshold")])
def test_bad_arguments_raise_before_any_device(kw, match):
    import torch_motion_correction_amd as mc

    raw, field = _raw_and_field()  # CPU tensors: no device is ever needed
    with pytest.raises(ValueError, match=match):
        mc.motion_correct_sum_raw(raw, None, field, 1.0, **kw)


@pytest.mark.parametrize("shape", [(3, 1, 1), (1, 3, 1, 1), (3, 3, 1, 1), (2, 3, 1, 1, 1), (2, 0, 1, 1)])
def test_bad_field_shapes_raise_before_any_device(shape):
    import torch_motion_correction_amd as mc

    raw, _ = _raw_and_field()
    with pytest.raises(ValueError, match="deformation_grid"):
        mc.motion_correct_sum_raw(raw, None, torch.zeros(shape), 1.0, dose_per_frame=1.0)


def test_gain_of_another_shape_raises_before_any_device():
    import torch_motion_correction_amd as mc

    raw, field = _raw_and_field()
    with pytest.raises(ValueError, match="gain"):
        mc.motion_correct_sum_raw(raw, torch.ones(64, 32), field, 1.0)


@pytest.mark.parametrize("dose", [-1.0, float("nan"), "x"])
def test_motion_correct_raw_checks_the_dose_before_any_device(dose):
    import torch_motion_correction_amd as mc

    raw, _ = _raw_and_field()
    with pytest.raises(ValueError, match="dose_per_frame"):
        mc.motion_correct_raw(raw, None, 1.0, dose_per_frame=dose)


def test_accumulate_entry_points_are_declared_and_exported():
    assert _lib.load().mc_abi_version() == 1
    for name, twin in (("mc_warp_rigid_raw_accumulate", "mc_warp_rigid_raw"),
                       ("mc_warp_frames_raw_accumulate", "mc_warp_frames_raw")):
        assert_entry_point(name)
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]  # the same arguments


def test_rigid_accumulate_validates_on_the_host():
    lib = _lib.load()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]

    def warp(raw=p[0], gain=p[1], mu=p[2], shifts=p[3], scratch=p[4], frames=p[5], total=p[6], st=U8, nf=4, phase=0):
        return lib.mc_warp_rigid_raw_accumulate(raw, st, gain, mu, nf, 256, 512, shifts, scratch, frames, total, phase,
                                                None)

    assert warp(total=None) == -1 and warp(frames=None, total=None) == -1  # out_sum is required
    assert warp(raw=None) == -1 and warp(gain=None) == -1 and warp(mu=None) == -1
    assert warp(shifts=None) == -1 and warp(scratch=None) == -1
    assert warp(st=7, total=None) == -1  # NULL arguments are refused before the storage type is looked at
    assert warp(nf=0) == -1 and warp(phase=3) == -1
    assert warp(st=2) == -2 and warp(st=3) == -2  # fp16 / fp32 frames: not the raw kernel's
    assert warp(raw=ctypes.c_void_p(0x10008)) == -2  # 16-byte aligned raw


def test_field_accumulate_validates_on_the_host():
    lib = _lib.load()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]

    def warp(st=U8, raw=p[0], gain=p[1], mu=p[2], lattice=p[3], nf=4, w=1024, GH=40, ps=1.0, scratch=p[4],
             frames=p[5], total=p[6]):
        return lib.mc_warp_frames_raw_accumulate(raw, st, gain, mu, nf, 1024, w, lattice, GH, 40, ps, scratch, frames,
                                                 total, None)

    assert warp(total=None) == -1 and warp(frames=None, total=None) == -1  # out_sum is required
    assert warp(raw=None) == -1 and warp(gain=None) == -1 and warp(mu=None) == -1
    assert warp(lattice=None) == -1 and warp(scratch=None) == -1
    assert warp(st=7, total=None) == -1
    assert warp(nf=0) == -1 and warp(ps=0.0) == -1
    assert warp(scratch=ctypes.c_void_p(0x40008)) == -1  # scratch is 16-byte aligned
    assert warp(st=2) == -2 and warp(st=3) == -2
    assert warp(w=1000) == -2 and warp(st=I16, w=1004) == -2
    assert warp(GH=1024) == -2  # a dense lattice: not the staged kernel's shape
