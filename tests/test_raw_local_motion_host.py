"""Host-side checks of the fused raw local-motion route (motion_correct_raw_patches, mc_xc_rows_forward_dual_raw,
mc_warp_frames_raw): the public signature, argument validation before any device is touched, and the C entry
points' own checks (no launch)."""

import ctypes
import inspect

import pytest
import torch

from torch_motion_correction_amd import _lib, plan

U8, I16, F16, F32 = 0, 1, 2, 3


def test_public_entry_point_and_defaults():
    import torch_motion_correction_amd as mc

    assert "motion_correct_raw_patches" in mc.__all__
    sig = inspect.signature(mc.motion_correct_raw_patches)
    assert list(sig.parameters)[:3] == ["movie", "gain", "pixel_spacing"]
    want = dict(patch_sidelength=1024, reference_frame=None, reference_strategy="mean_except_current", b_factor=500,
                frequency_range=(300, 10), sub_pixel_refinement=True, temporal_smoothing=True,
                smoothing_window_size=5, deformation_field=None, outlier_rejection=True, outlier_threshold=3.0,
                grid_type="catmull_rom", mean_zero=True, return_frames=False, device=None, hot_pixel_threshold=None,
                return_hot_counts=False)
    got = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert got == want


@pytest.mark.parametrize("kw,match", [(dict(reference_strategy="median"), "reference_strategy"),
                                      (dict(hot_pixel_threshold=0.0), "hot_pixel_threshold"),
                                      (dict(hot_pixel_threshold=float("nan")), "hot_pixel_threshold"),
                                      (dict(hot_pixel_threshold="ten"), "hot_pixel_threshold"),
                                      (dict(patch_sidelength=0), "patch_sidelength")])
def test_bad_arguments_raise_before_any_device(kw, match):
    import torch_motion_correction_amd as mc

    raw = torch.zeros((2, 64, 64), dtype=torch.uint8)  # CPU tensors: no device is ever needed
    with pytest.raises(ValueError, match=match):
        mc.motion_correct_raw_patches(raw, None, 1.0, **kw)


def test_new_entry_points_are_exported():
    lib = _lib.load()
    for name in ("mc_xc_rows_forward_dual_raw", "mc_warp_frames_raw"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None


def test_raw_patch_rows_validate_on_the_host():
    lib = _lib.load()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(12)]
    g1024 = plan.xc_geometry(1024, 1024, 0.1, 16, 8)
    g512 = plan.xc_geometry(512, 512, 0.1, 16, 8)
    gk3 = plan.xc_geometry(4092, 5760, 0.1, 16, 8)

    def k1(st=U8, raw=p[0], gain=p[1], area=4092 * 5760, g=g1024, T1a=p[8], expo_b=p[4], T1b=p[9], sub=p[6],
           njobs=2):
        return lib.mc_xc_rows_forward_dual_raw(raw, st, gain, area, p[2], 5760, p[3], expo_b, p[5], sub, p[7], T1a,
                                               T1b, p[10], njobs, g, None, None)

    assert k1(st=F32) == -2 and k1(st=F16) == -2 and k1(st=9) == -2
    assert k1(raw=None) == -1 and k1(gain=None) == -1 and k1(sub=None) == -1 and k1(T1a=None) == -1
    assert k1(T1b=None) == -1  # a second exponent without its output
    assert k1(area=0) == -1 and k1(njobs=0) == -1
    assert k1(g=g512) == -2 and k1(g=gk3) == -2  # the wave-per-row 1024-sample engine only
    assert k1(st=I16, raw=ctypes.c_void_p(0x10001), expo_b=None, T1b=None) == -2  # i16 rows are 2-byte aligned


def test_raw_field_warp_validates_on_the_host():
    lib = _lib.load()
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]

    def warp(st=U8, raw=p[0], gain=p[1], mu=p[2], nf=4, h=1024, w=1024, GH=40, GW=40, ps=1.0, scratch=p[4],
             frames=p[5], total=p[6]):
        return lib.mc_warp_frames_raw(raw, st, gain, mu, nf, h, w, p[3], GH, GW, ps, scratch, frames, total, None)

    assert warp(st=F32) == -2 and warp(st=F16) == -2 and warp(st=9) == -2
    assert warp(raw=None) == -1 and warp(gain=None) == -1 and warp(mu=None) == -1 and warp(scratch=None) == -1
    assert warp(frames=None, total=None) == -1
    assert warp(nf=0) == -1 and warp(h=1) == -1 and warp(ps=0.0) == -1
    assert warp(scratch=ctypes.c_void_p(0x40008)) == -1  # scratch is 16-byte aligned
    assert warp(w=1000) == -2              # u8 rows of whole 16-sample units only
    assert warp(st=I16, w=1004) == -2
    assert warp(raw=ctypes.c_void_p(0x10008)) == -2  # 16-byte aligned raw
    assert warp(GH=1024) == -2             # a dense lattice: not the staged kernel's shape
