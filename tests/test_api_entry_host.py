"""The device prelude of the API entry points (_lib.gpu_entry) and the order "argument rules, then the GPU" without a
GPU: the prelude's rule with torch.cuda's probes replaced by recorders; the entry points that check their arguments
first (each raises its own exception where no GPU is visible); the entry points whose body opens with the prelude (each
needs a GPU before any of its own checks runs)."""

import pytest
import torch


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


# ------------------------------------------------------------------ 1. the prelude's rule

CURRENT = 3  # the fake current device: distinguishable from an index a caller names


@pytest.fixture
def scopes(monkeypatch):
    """torch.cuda with a GPU "visible", device CURRENT current and torch.cuda.device recording -> the event list."""
    events = []

    class Scope:
        def __init__(self, device):
            self.device = device

        def __enter__(self):
            events.append(("enter", self.device))

        def __exit__(self, *exc):
            events.append(("exit", self.device))
            return False

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: CURRENT)
    monkeypatch.setattr(torch.cuda, "device", Scope)
    return events


CUR = torch.device("cuda", CURRENT)
PRELUDE_CASES = [  # (first, device, out_dev, dev)
    pytest.param(torch.zeros(2), None, torch.device("cpu"), CUR, id="none-cpu-tensor"),
    pytest.param(torch.zeros(2), "cuda", torch.device("cuda"), CUR, id="cuda"),
    pytest.param(torch.zeros(2), "cuda:1", torch.device("cuda", 1), torch.device("cuda", 1), id="cuda:1"),
    pytest.param(torch.zeros(2), "cpu", torch.device("cpu"), CUR, id="cpu"),
    pytest.param([1.0, 2.0], None, CUR, CUR, id="non-tensor"),
]


@pytest.mark.parametrize("first, device, out_dev, dev", PRELUDE_CASES)
def test_prelude_rule(scopes, first, device, out_dev, dev):
    from torch_motion_correction_amd._lib import gpu_entry

    with gpu_entry(first, device) as pair:
        assert pair == (out_dev, dev)
        assert all(isinstance(d, torch.device) for d in pair)
        assert scopes == [("enter", dev)]
    assert scopes == [("enter", dev), ("exit", dev)]


@pytest.mark.parametrize("first, device, out_dev, dev", PRELUDE_CASES)
def test_prelude_leaves_the_scope_when_the_body_raises(scopes, first, device, out_dev, dev):
    from torch_motion_correction_amd._lib import gpu_entry

    with pytest.raises(KeyError, match="body"):
        with gpu_entry(first, device):
            raise KeyError("body")
    assert scopes == [("enter", dev), ("exit", dev)]


@pytest.mark.parametrize("first, device, out_dev, dev", PRELUDE_CASES)
def test_prelude_without_a_gpu_enters_no_scope(mc, scopes, monkeypatch, first, device, out_dev, dev):
    from torch_motion_correction_amd._lib import gpu_entry

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ran = []
    with pytest.raises(mc.McorrError, match="no CPU fallback"):
        with gpu_entry(first, device):
            ran.append(1)
    assert scopes == [] and ran == []


# ------------------------------------------------------------------ 2. argument rules first, then the GPU

U8 = torch.zeros(3, 8, 8, dtype=torch.uint8)
F32 = torch.zeros(3, 8, 8)
RIGID = torch.zeros(2, 3, 1, 1)
LOCAL = torch.zeros(2, 3, 2, 2)
CROP_U8 = torch.zeros(2, 512, 128, dtype=torch.uint8)

CHECKS_FIRST = [  # (function, args, kwargs, exception, message fragment): one row per function, one broken rule each
    ("refine_global_motion", (torch.zeros(4, 8), 1.0), {}, ValueError, r"image must be \(t, h, w\)"),
    ("refine_global_motion_raw", (U8, None, 1.0), dict(reference_frame=7), IndexError, "out of bounds"),
    ("refine_local_motion", (F32, 1.0), dict(patch_sidelength=16), ValueError, "exceeds the frame size"),
    ("refine_local_motion_raw", (U8, torch.zeros(4, 4), 1.0), dict(patch_sidelength=8), ValueError,
     "gain reference has shape"),
    ("motion_correct_raw", (U8, None, 1.0), dict(dose_per_frame=-1.0), ValueError,
     "dose_per_frame must be a finite number"),
    ("motion_correct_raw_patches", (U8, None, 1.0), dict(reference_strategy="nope"), ValueError,
     "Unknown reference_strategy"),
    ("motion_correct_sum_raw", (U8, None, torch.zeros(2, 3, 1), 1.0), {}, ValueError,
     r"deformation_grid must be a \(2, nt, gh, gw\) tensor"),
    ("motion_correct_sum_fast", (F32, LOCAL, 1.0), {}, ValueError, "Expected single patch deformation field"),
    ("motion_correct_sum_fast_raw", (U8, None, torch.zeros(2, 4, 1, 1), 1.0), {}, ValueError,
     "4 time points, the movie 3 frames"),
    ("motion_correct_raw_fast", (U8, None, 1.0), dict(return_plain_sum=True), ValueError,
     "return_plain_sum needs dose_per_frame"),
    ("fourier_crop", (torch.zeros(512, 128),), dict(binning=3), ValueError, "binning must be 2"),
    ("fourier_crop_raw", (torch.zeros(2, 10, 12, dtype=torch.uint8), None), {}, NotImplementedError,
     "the Fourier crop needs"),
    ("motion_correct_raw_binned", (CROP_U8, None, 1.0),
     dict(patch_sidelength=64, dose_per_frame=1.0, return_plain_sum=True), ValueError,
     "belongs to the whole-image route"),
    ("group_frames_raw", (F32, 2), {}, ValueError, "movie must be a uint8 or int16 tensor"),
    ("motion_correct_raw_grouped", (U8, None, 1.0, 0), {}, ValueError, "group must be an int >= 1"),
    ("correct_magnification_distortion", (torch.zeros(8, 8), 1.5, 1.0, 0.0), {}, ValueError,
     "major_scale must lie in"),
]


@pytest.mark.parametrize("name, args, kwargs, exc, fragment", CHECKS_FIRST, ids=[r[0] for r in CHECKS_FIRST])
def test_argument_rules_are_raised_before_the_gpu_is_asked_for(mc, monkeypatch, name, args, kwargs, exc, fragment):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(exc, match=fragment) as info:
        getattr(mc, name)(*args, **kwargs)
    assert not isinstance(info.value, mc.McorrError)


@pytest.mark.parametrize("name, args, kwargs", [
    ("refine_global_motion", (F32, 1.0), {}),
    ("motion_correct_sum_fast_raw", (U8, None, RIGID, 1.0), {}),
    ("correct_magnification_distortion", (torch.zeros(8, 8), 1.01, 1.0, 0.0), {}),
])
def test_checks_first_functions_need_a_gpu_once_the_arguments_pass(mc, monkeypatch, name, args, kwargs):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(mc.McorrError, match="no CPU fallback"):
        getattr(mc, name)(*args, **kwargs)


# ------------------------------------------------------------------ 3. the GPU first, then the body's own rules

GPU_FIRST = [  # (function, args, kwargs, what the body would refuse): one row per function
    ("evaluate_deformation_field", (LOCAL, torch.zeros(5, 3)), dict(grid_type="nope"), "grid_type"),
    ("evaluate_deformation_field_at_t", (LOCAL, 0.5, (4, 4)), dict(grid_type="nope"), "grid_type"),
    ("resample_deformation_field", (LOCAL, (3,)), {}, "a resolution of one number"),
    ("estimate_global_motion", (F32, 1.0), dict(reference_frame=7), "reference_frame out of range"),
    ("estimate_motion_cross_correlation_patches", (F32, 1.0), dict(reference_strategy="nope"), "reference_strategy"),
    ("correct_motion", (F32, LOCAL, 1.0), dict(grad=True), "grad=True"),
    ("correct_motion_two_grids", (F32, object(), object(), 1.0), {}, "grids without .data"),
    ("correct_motion_slow", (F32, LOCAL), dict(grad=True), "grad=True"),
    ("motion_correct_sum", (F32, LOCAL, 1.0), dict(grid_type="nope"), "grid_type"),
    ("condition_movie", (U8,), dict(hot_pixel_threshold=-1.0), "hot_pixel_threshold"),
    ("dose_weighted_sum", (F32, 1.0, "much"), {}, "dose_per_frame"),
    ("estimate_local_motion", (F32, 1.0, (4, 4), (3, 2, 2)), dict(grid_type="nope"), "grid_type"),
    ("correct_motion_fast", (F32, LOCAL), {}, "a field with more than one patch"),
    ("get_pixel_shifts", (torch.zeros(8, 8), 1.0, torch.zeros(2, 2, 2)), dict(pixel_grid=torch.zeros(4, 3)),
     "pixel_grid's last axis"),
]


@pytest.mark.parametrize("name, args, kwargs, refused", GPU_FIRST, ids=[r[0] for r in GPU_FIRST])
def test_directly_scoped_functions_need_a_gpu_before_their_own_checks(mc, monkeypatch, name, args, kwargs, refused):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(mc.McorrError, match="no CPU fallback"):
        getattr(mc, name)(*args, **kwargs)
