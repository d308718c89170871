"""The device rule of every API entry point that computes under _lib.gpu_entry, on the GPU: a CPU input comes back on
the CPU, bit for bit the .cpu() of the same call on device-resident inputs; ``device="cuda"`` returns on the GPU; the
current device is the same afterwards.  Inputs are the smallest the functions' own GPU tests use."""

import random

import pytest
import torch

from conftest import blob_stack, ramp_field

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def _gen(seed):
    return torch.Generator().manual_seed(seed)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def stack(shape, seed=3):
    return _cached(("stack", shape, seed), lambda: torch.randn(*shape, generator=_gen(seed)))


def raw_u8(shape, seed=4):
    """(u8 movie, gain of 1 +- 0.1) of random counts."""
    def make():
        g = _gen(seed)
        movie = (torch.rand(*shape, generator=g) * 40).to(torch.uint8)
        return movie, 1.0 + 0.1 * (2 * torch.rand(*shape[1:], generator=g) - 1)
    return _cached(("raw", shape, seed), make)


def field(shape, amp=1.5, seed=5):
    return amp * (2 * torch.rand(2, *shape, generator=_gen(seed)) - 1)  # fresh: correct_motion_fast negates its grid


SPLINE = (4, 3, 5)  # test_gpu_parity.test_spline_lattice_and_points
RAW = (6, 1024, 1024)  # test_raw_fast_sums, test_frame_groups: the raw kernels' 1024-px rows and patches
SMALL_RAW = (6, 96, 120)  # test_global_refine's chirp-z shape: the raw routes condition the movie
CROP = (5, 512, 1024)  # test_fourier_crop.SHAPES[0]

# name -> () -> (args, kwargs) on the CPU; `device` says whether the function takes ``device=``
CASES = {
    "evaluate_deformation_field": (lambda: ((field(SPLINE), torch.rand(4, 6, 3, generator=_gen(6))), {}), False),
    "evaluate_deformation_field_at_t": (lambda: ((field(SPLINE), 0.37, (30, 50)), {}), False),
    "resample_deformation_field": (lambda: ((field(SPLINE), (6, 4, 7)), {}), False),
    "get_pixel_shifts": (lambda: ((torch.zeros(64, 96), 1.7, torch.randn(2, 20, 30, generator=_gen(7))), {}), False),
    "estimate_global_motion": (lambda: ((blob_stack(True), 1.0), {}), True),
    "estimate_motion_cross_correlation_patches": (lambda: ((blob_stack(True), 1.0), dict(patch_sidelength=32)), True),
    "correct_motion": (lambda: ((blob_stack(True), ramp_field(), 1.0), {}), True),
    "correct_motion_two_grids": (lambda: ((blob_stack(False), ramp_field(), torch.zeros(2, 5, 2, 2), 1.0),
                                          dict(grad=False)), True),
    "correct_motion_slow": (lambda: ((blob_stack(False), ramp_field()), {}), True),
    "correct_motion_fast": (lambda: ((blob_stack(False), ramp_field(g=1)), {}), True),
    "motion_correct_sum": (lambda: ((blob_stack(True), ramp_field(), 1.0), dict(return_frames=True)), True),
    "condition_movie": (lambda: (raw_u8((3, 70, 90)), dict(hot_pixel_threshold=10.0, return_hot_counts=True)), True),
    "dose_weighted_sum": (lambda: ((stack((3, 64, 75)), 1.0, 1.2), {}), True),
    "estimate_local_motion": (lambda: ((blob_stack(True), 1.0, (32, 32), (5, 2, 2)), dict(n_iterations=2)), True),
    "refine_global_motion": (lambda: ((stack(SMALL_RAW), 1.0), dict(max_iterations=2)), True),
    "refine_global_motion_raw": (lambda: ((*raw_u8(SMALL_RAW), 1.0), dict(max_iterations=2)), True),
    "refine_local_motion": (lambda: ((stack((6, 200, 240)), 1.0), dict(patch_sidelength=96, max_iterations=2)), True),
    "refine_local_motion_raw": (lambda: ((*raw_u8((6, 200, 240)), 1.0), dict(patch_sidelength=96, max_iterations=2)),
                                True),
    "motion_correct_raw": (lambda: ((*raw_u8(RAW), 1.0), dict(return_hot_counts=True)), True),
    "motion_correct_raw_patches": (lambda: ((*raw_u8(RAW), 1.0), {}), True),
    "motion_correct_sum_raw": (lambda: ((*raw_u8(RAW), field((6, 2, 2)), 1.0),
                                        dict(dose_per_frame=1.0, return_plain_sum=True)), True),
    "motion_correct_sum_fast": (lambda: ((stack((3, 64, 128)), field((3, 1, 1)), 1.0), {}), True),
    "motion_correct_sum_fast_raw": (lambda: ((*raw_u8(RAW), field((6, 1, 1)), 1.0),
                                             dict(dose_per_frame=1.0, return_plain_sum=True)), True),
    "motion_correct_raw_fast": (lambda: ((*raw_u8(RAW), 1.0), dict(return_hot_counts=True)), True),
    "fourier_crop": (lambda: ((stack((2, 512, 128)),), {}), True),
    "fourier_crop_raw": (lambda: (raw_u8(CROP), dict(return_hot_counts=True)), True),
    "motion_correct_raw_binned": (lambda: ((*raw_u8(CROP), 0.5), {}), True),
    "group_frames_raw": (lambda: ((raw_u8((5, 3, 8))[0], 3), {}), True),
    "motion_correct_raw_grouped": (lambda: ((*raw_u8(RAW), 1.0, 3), dict(dose_per_frame=1.0, return_plain_sum=True)),
                                   True),
    "motion_correct_raw_grouped-patches": (lambda: ((*raw_u8(RAW), 1.0, 3),
                                                    dict(patch_sidelength=1024, dose_per_frame=1.0)), True),
    "correct_magnification_distortion": (lambda: ((stack((2, 33, 47)), 1.02, 0.98, 30.0), {}), True),
}


def _to(x, dev):
    return x.to(dev) if isinstance(x, torch.Tensor) else x


def _tensors(res):
    res = res if isinstance(res, tuple) else (res,)
    assert res and all(isinstance(r, torch.Tensor) for r in res)
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_device_rule(mc, dev, name):
    make, takes_device = CASES[name]
    fn = getattr(mc, name.split("-")[0])

    def call(on, **extra):
        args, kwargs = make()
        random.seed(7)  # estimate_local_motion shuffles its patches
        return _tensors(fn(*(_to(a, on) for a in args), **{k: _to(v, on) for k, v in kwargs.items()}, **extra))

    before = torch.cuda.current_device()
    on_cpu = call("cpu")
    on_gpu = call(dev)
    assert len(on_cpu) == len(on_gpu)
    for a, b in zip(on_cpu, on_gpu):
        assert a.device.type == "cpu" and b.device == dev
        assert a.dtype == b.dtype and torch.equal(a, b.cpu())
    if takes_device:
        for a, c in zip(on_cpu, call("cpu", device="cuda")):
            assert c.device.type == "cuda" and torch.equal(a, c.cpu())
    assert torch.cuda.current_device() == before
