"""Rolling frame-group sums (group_frames_raw, motion_correct_raw_grouped), without a GPU: the names and parameter
lists, the header and the ctypes table on mc_raw_group_frames, every argument rule before any device is touched, the
entry point's host checks with fake pointers, the window rule's restatement (tests/group_reference.py) on hand-made
cases, and the kernel's per-thread body run thread by thread on the CPU under the address and undefined-behaviour
sanitizers (tests/host_raw_group.cpp, a stand-alone program started as a child process)."""

import ctypes
import inspect

import numpy as np
import pytest
import torch

import group_reference as gr
from kernel_harness import assert_entry_point, run_host_program
import torch_motion_correction_amd as mc
from torch_motion_correction_amd import _lib, api



def test_names_and_parameter_lists():
    for name in ("group_frames_raw", "motion_correct_raw_grouped"):
        assert name in mc.__all__ and getattr(mc, name) is getattr(api, name)
    sig = inspect.signature(mc.group_frames_raw)
    assert list(sig.parameters) == ["movie", "group", "device"] and sig.parameters["device"].default is None
    assert sig.parameters["group"].default is inspect.Parameter.empty
    sig = inspect.signature(mc.motion_correct_raw_grouped)
    assert list(sig.parameters) == [
        "movie", "gain", "pixel_spacing", "group", "patch_sidelength", "reference_frame", "b_factor", "frequency_range",
        "grid_type", "mean_zero", "dose_per_frame", "pre_exposure", "voltage", "return_plain_sum", "device"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(patch_sidelength=None, reference_frame=None, b_factor=500, frequency_range=(300, 10),
                            grid_type="catmull_rom", mean_zero=True, dose_per_frame=None, pre_exposure=0.0,
                            voltage=300.0, return_plain_sum=False, device=None)
    assert "hot_pixel_threshold" not in sig.parameters


def test_header_and_signatures_agree_on_the_entry_point():
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    assert_entry_point("mc_raw_group_frames", [vp, i32, i32, i32, i32, i32, vp, vp, vp])


def test_the_object_is_in_the_build():
    assert_entry_point("mc_raw_group_frames", source=("raw_group.hip", "raw_group", []))


def test_entry_point_validates_on_the_host():
    """Fake pointers and a null stream: every call below must answer before it launches anything."""
    lib = _lib.load()
    p = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(3)]
    ARG, UNSUPPORTED = -1, -2

    def call(raw=p[0], storage=0, t=4, h=8, w=8, g=3, out=p[1], flag=p[2]):
        return lib.mc_raw_group_frames(raw, storage, t, h, w, g, out, flag, None)

    for name in ("raw", "out", "flag"):
        assert call(**{name: None}) == ARG, name
    assert call(t=0) == ARG and call(t=-2) == ARG and call(g=0) == ARG and call(g=-1) == ARG
    assert call(h=0) == ARG and call(w=0) == ARG
    for storage in (2, 3, 4, -1):  # fp16 / fp32 movies and unknown kinds have no kernel
        assert call(storage=storage) == UNSUPPORTED, storage
    # the window is min(g, t) frames: u8 up to 128, i16 up to 32768
    assert call(t=200, g=129) == UNSUPPORTED and call(t=129, g=2**31 - 1) == UNSUPPORTED
    assert call(storage=1, t=40000, g=32769) == UNSUPPORTED
    assert call(storage=1, raw=ctypes.c_void_p(0x100001)) == ARG  # an i16 movie at an odd address
    assert call(out=ctypes.c_void_p(0x200001)) == ARG and call(flag=ctypes.c_void_p(0x300002)) == ARG
    assert call(h=1 << 30, w=1 << 30) == ARG  # more pieces than a grid holds


# ------------------------------------------------------------------ argument rules, devices refused


def _refuse_devices(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    monkeypatch.setattr(api, "require_gpu", refuse)
    monkeypatch.setattr(api, "device_scope", refuse)


def test_argument_rules_hold_before_any_device_is_touched(monkeypatch):
    _refuse_devices(monkeypatch)
    u8 = torch.zeros(6, 8, 16, dtype=torch.uint8)
    gain = torch.ones(8, 16)
    calls = (lambda m, g: mc.group_frames_raw(m, g), lambda m, g: mc.motion_correct_raw_grouped(m, gain, 1.0, g))
    for call in calls:
        for bad in (0, -1, 2.0, None, True, "3"):
            with pytest.raises(ValueError, match="group must be an int >= 1"):
                call(u8, bad)
        with pytest.raises(ValueError, match="128"):  # a u8 window of 129 frames
            call(torch.zeros(200, 8, 16, dtype=torch.uint8), 129)
        with pytest.raises(ValueError, match="128"):  # min(group, t) counts
            call(torch.zeros(129, 8, 16, dtype=torch.uint8), 1000)
        for movie in (torch.zeros(6, 8, 16), torch.zeros(6, 8, 16, dtype=torch.float16),
                      torch.zeros(6, 8, 16, dtype=torch.int32)):
            with pytest.raises(ValueError, match="uint8 or int16"):
                call(movie, 3)
        for movie in (torch.zeros(8, 16, dtype=torch.uint8), torch.zeros(1, 6, 8, 16, dtype=torch.uint8),
                      torch.zeros(0, 8, 16, dtype=torch.uint8), np.zeros((6, 8, 16), dtype=np.uint8)):
            with pytest.raises(ValueError, match=r"\(t, h, w\)"):
                call(movie, 3)
    with pytest.raises(ValueError, match="32768"):  # an i16 window of 32769 frames (an expanded view: no memory)
        mc.group_frames_raw(torch.zeros(1, 1, 1, dtype=torch.int16).expand(32769, 1, 1), 40000)
    for bad_gain in (torch.ones(16, 8), torch.ones(8, 15), torch.ones(6, 8, 16)):
        with pytest.raises(ValueError, match="gain reference has shape"):
            mc.motion_correct_raw_grouped(u8, bad_gain, 1.0, 3)
    with pytest.raises(ValueError, match="whole-image route"):
        mc.motion_correct_raw_grouped(u8, gain, 1.0, 3, patch_sidelength=1024, dose_per_frame=1.0,
                                      return_plain_sum=True)
    with pytest.raises(ValueError, match="return_plain_sum needs dose_per_frame"):
        mc.motion_correct_raw_grouped(u8, gain, 1.0, 3, return_plain_sum=True)
    for bad_dose in (-1.0, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError, match="dose_per_frame must be"):
            mc.motion_correct_raw_grouped(u8, gain, 1.0, 3, dose_per_frame=bad_dose)
    for bad_patch in (0, -4):
        with pytest.raises(ValueError, match="patch_sidelength must be > 0"):
            mc.motion_correct_raw_grouped(u8, gain, 1.0, 3, patch_sidelength=bad_patch)


# ------------------------------------------------------------------ the window rule, by hand


def test_window_rule_on_hand_made_cases():
    one = np.array([[[7, 9]]], dtype=np.uint8)  # t = 1: every group is the frame itself
    for g in (1, 2, 3, 100):
        assert np.array_equal(gr.group_frames(one, g), [[[7, 9]]])
    ramp = np.arange(1, 6, dtype=np.uint8).reshape(5, 1, 1)  # frames 1 2 3 4 5
    col = lambda a: np.asarray(a, dtype=np.int64).reshape(-1, 1, 1)  # noqa: E731
    assert np.array_equal(gr.group_frames(ramp, 1), col([1, 2, 3, 4, 5]))  # g = 1: the movie
    # g = 2 is asymmetric: no frame before, one after -> 1+2, 2+3, 3+4, 4+5, 5
    assert np.array_equal(gr.group_frames(ramp, 2), col([3, 5, 7, 9, 5]))
    # g = 3: one before, one after -> 1+2, 1+2+3, 2+3+4, 3+4+5, 4+5
    assert np.array_equal(gr.group_frames(ramp, 3), col([3, 6, 9, 12, 9]))
    # g = 4: one before, two after -> 1+2+3, 1+2+3+4, 2+3+4+5, 3+4+5, 4+5
    assert np.array_equal(gr.group_frames(ramp, 4), col([6, 10, 14, 12, 9]))
    # g = t = 5: two before, two after -> 6, 10, 15, 14, 12
    assert np.array_equal(gr.group_frames(ramp, 5), col([6, 10, 15, 14, 12]))
    # g > 2 t: every window is the whole movie
    for g in (11, 13, 1000):
        assert np.array_equal(gr.group_frames(ramp, g), col([15] * 5))
    assert [gr.group_window(i, 5, 2) for i in range(5)] == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 4)]
    assert gr.interior_frames(16, 5) == list(range(2, 14)) and gr.interior_frames(5, 2) == [0, 1, 2, 3]
    # signed input and sums beyond int16 stay exact in the restatement
    neg = np.full((3, 1, 2), -32768, dtype=np.int16)
    assert np.array_equal(gr.group_frames(neg, 3)[:, 0, 0], [-65536, -98304, -65536])
    assert gr.group_frames(neg, 3).dtype == np.int64


# ------------------------------------------------------------------ the kernel's body on the CPU, sanitized


def test_kernel_body_on_the_host_under_sanitizers(tmp_path):
    """csrc/raw_group.h -- the per-thread body raw_group.hip compiles for the device -- is built for the host with
    -fsanitize=address,undefined into a program of its own and run as a child process: every thread of every
    workgroup in turn on exactly-sized heap buffers, vector and element path, u8 and i16, the shapes and groups of
    tests/test_frame_groups.py, the int16 edge and the overflow flag, against a naive loop.  Nothing sanitized is
    loaded into this process.  Needs clang++ (ext_vector_type, __builtin_nontemporal_*); the ROCm one is used."""
    res = run_host_program("host_raw_group.cpp", tmp_path)
    assert res.stdout.count(" path: ok") == 92
