"""Iterative sub-pixel patch alignment, without a GPU: the float64 restatement (tests/local_refine_reference.py)
recovers planted local motion that a rigid field cannot, the damped update does not oscillate for two frames, the
window-offset rule keeps every window inside the frame; the public functions exist with their parameter lists and
check their arguments before any device is touched; the header and the ctypes table agree on the new entry points."""

import ctypes
import inspect

import numpy as np
import pytest
import torch

import global_refine_reference as gr
import local_refine_reference as lr
from kernel_harness import assert_entry_point, header_parameters
import torch_motion_correction_amd as mc
from torch_motion_correction_amd import _lib, engine

SHAPE, P = (6, 384, 512), 128


def planted_motion(t):
    """Rigid drift with fractions plus a local part that changes by up to 0.6 px (y) and 1.2 px (x) from the left to
    the right edge of the frame, relative to the middle frame."""
    f = np.arange(t) - t // 2
    rigid = np.stack([np.linspace(-3.3, 4.6, t), np.linspace(2.7, -1.9, t)], axis=1)
    slope = np.stack([0.6 * np.sin(0.8 * f), -1.2 * f / (t // 2)], axis=1)
    return rigid - rigid[t // 2], slope


@pytest.fixture(scope="module")
def planted():
    t = SHAPE[0]
    rigid, slope = planted_motion(t)
    # 128-px patches (a mask of 32 px radius) hold less than one period of the slowest waves of the default
    # texture band: the texture here starts at 0.04 cycles/px
    movie, drift = lr.planted_local_movie(*SHAPE, rigid, slope, noise=0.25, seed=3, band=(0.04, 0.12))
    return movie, lr.planted_truth(drift, SHAPE, P)


def as_shifts(field):
    t = field.shape[1]
    return field.permute(1, 2, 3, 0).reshape(t, -1, 2).double().numpy()


def test_restatement_recovers_planted_local_motion(planted):
    movie, truth = planted
    field, info = lr.refine_local_motion(movie, 1.0, P, max_iterations=5, convergence_threshold=0.0, details=True)
    t, gh, gw = SHAPE[0], 4, 6
    assert tuple(field.shape) == (2, t, gh, gw) and field.dtype == torch.float64
    err = float(np.abs(as_shifts(field) - truth).max())
    rigid_err = float(np.abs(info["start"] - truth).max())  # the start: the refined rigid field
    print(f"refined {err:.4f} px, rigid start {rigid_err:.4f} px, max|r| {info['history']}")
    assert len(info["history"]) == 5
    assert err <= 0.1, err
    assert rigid_err >= 0.3, rigid_err
    assert not field[:, t // 2].any()  # the reference frame is the coordinate system, in every patch


def test_two_frames_do_not_oscillate():
    """With t = 2 each patch sees the other frame's whole error: the factor (t - 1)/t halves the update and max |r|
    falls; an undamped update overshoots by the full residual and never does."""
    shape, p = (2, 256, 384), 128
    movie, _ = lr.planted_local_movie(*shape, [[0.0, 0.0], [0.4, -0.3]], [[0.0, 0.0], [0.2, 0.3]], noise=0.25, seed=5)
    s0 = np.zeros((2, len(lr.patch_lattice(shape, p)[2]), 2))
    o = lr.window_offsets(s0, shape, p)
    S = lr.patch_spectra(movie, 1.0, p, o)
    _, damped, _, _ = lr.refine_patches(S, p, s0, o, max_iterations=4, threshold=0.0)
    _, undamped, _, _ = lr.refine_patches(S, p, s0, o, max_iterations=4, threshold=0.0, damping=1.0)
    print(damped, undamped)
    assert damped[-1] < 0.01 < undamped[-1], (damped, undamped)


@pytest.mark.parametrize("shape,p", [((5, 384, 512), 128), ((3, 200, 240), 96), ((4, 1536, 2048), 1024),
                                     ((2, 256, 256), 256)])
def test_offset_rule_keeps_every_window_inside_the_frame(shape, p):
    t, h, w = shape
    cy, cx, origin = engine.patch_origins(shape, p)
    npatch = len(cy) * len(cx)
    assert origin.shape == (npatch, 2) and np.array_equal(origin, lr.patch_lattice(shape, p)[2])
    g = torch.Generator().manual_seed(h + p)
    start = (80 * torch.rand(t, npatch, 2, generator=g) - 40).float()
    start[0] = 40.0
    start[-1] = -40.0
    start[0, 0] = torch.tensor([2.5, -3.5])  # halves round to even
    o = engine.refine_window_offsets(start, shape, p)
    assert o.dtype == torch.int64 and tuple(o.shape) == (t, npatch, 2)
    corner = torch.as_tensor(origin)[None] + o
    assert int(corner.min()) >= 0
    assert int(corner[..., 0].max()) <= h - p and int(corner[..., 1].max()) <= w - p
    # inside the frame the offset is the start rounded half to even; the two sides use the same rule
    assert np.array_equal(o.numpy(), lr.window_offsets(start.double().numpy(), shape, p))
    free = (corner[..., 0] > 0) & (corner[..., 0] < h - p) & (corner[..., 1] > 0) & (corner[..., 1] < w - p)
    assert torch.equal(o[free], torch.round(start[free]).long())
    if len(cy) >= 3 and len(cx) >= 3:
        assert bool(free.any())  # interior patches move freely
    if p < min(h, w):
        assert tuple(o[0, 0].tolist()) == (2, 0)  # 2.5 -> 2; -3.5 -> -4, clamped at the frame's left edge
    else:
        assert not o.any()  # one patch as large as the frame: every window stays where it is


# ------------------------------------------------------------------ the public functions

COMMON = ["patch_sidelength", "deformation_field", "reference_frame", "b_factor", "frequency_range", "max_iterations",
          "convergence_threshold", "return_history", "device"]
DEFAULTS = dict(patch_sidelength=1024, deformation_field=None, reference_frame=None, b_factor=500,
                frequency_range=(300, 10), max_iterations=10, convergence_threshold=0.01, return_history=False,
                device=None, mean_zero=True, hot_pixel_threshold=None)


def test_functions_are_exported_with_their_parameter_lists():
    for name in ("refine_local_motion", "refine_local_motion_raw"):
        assert callable(getattr(mc, name)) and name in mc.__all__
    sig = inspect.signature(mc.refine_local_motion)
    assert list(sig.parameters) == ["image", "pixel_spacing"] + COMMON
    raw = inspect.signature(mc.refine_local_motion_raw)
    assert list(raw.parameters) == ["movie", "gain", "pixel_spacing"] + COMMON + ["mean_zero", "hot_pixel_threshold"]
    for s in (sig, raw):
        for k, v in s.parameters.items():
            if k in DEFAULTS:
                assert v.default == DEFAULTS[k], k
            else:
                assert v.default is inspect.Parameter.empty, k
    assert callable(engine.refine_patch_shifts) and callable(engine.refine_window_offsets)
    assert list(inspect.signature(engine.refine_patch_shifts).parameters) == [
        "spectra", "shape", "pl", "p", "start_px", "reference_frame", "max_iterations", "threshold"]


def _refuse_devices(monkeypatch):
    from torch_motion_correction_amd import api

    def refuse(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    monkeypatch.setattr(api, "require_gpu", refuse)
    monkeypatch.setattr(api, "device_scope", refuse)


def _argument_rules(call, what):
    with pytest.raises(ValueError, match=f"{what} must be"):
        call(bad_movie=True)
    for bad in (0, -1, 2.5, True, None, "3"):
        with pytest.raises(ValueError, match="max_iterations"):
            call(max_iterations=bad)
    for bad in (-0.1, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="convergence_threshold"):
            call(convergence_threshold=bad)
    for bad in (4, -5):
        with pytest.raises(IndexError):
            call(reference_frame=bad)
    for bad in (0, -8, 65, "x"):
        with pytest.raises(ValueError, match="patch_sidelength"):
            call(patch_sidelength=bad)
    for bad in (torch.zeros(4, 2), torch.zeros(3, 4, 1, 1), torch.zeros(2, 0, 1, 1), "field"):
        with pytest.raises(ValueError, match="deformation_field must be"):
            call(deformation_field=bad)


def test_refine_local_motion_argument_rules(monkeypatch):
    _refuse_devices(monkeypatch)
    img = torch.zeros(4, 64, 64)

    def call(bad_movie=False, patch_sidelength=32, **kw):
        return mc.refine_local_motion(img[0] if bad_movie else img, 1.0, patch_sidelength, **kw)

    _argument_rules(call, "image")
    with pytest.raises(NotImplementedError, match="512"):
        mc.refine_local_motion(torch.zeros(513, 8, 8), 1.0, 8)


def test_refine_local_motion_raw_argument_rules(monkeypatch):
    _refuse_devices(monkeypatch)
    raw = torch.zeros(4, 64, 64, dtype=torch.uint8)

    def call(bad_movie=False, patch_sidelength=32, **kw):
        return mc.refine_local_motion_raw(raw[0] if bad_movie else raw, None, 1.0, patch_sidelength, **kw)

    _argument_rules(call, "movie")
    with pytest.raises(ValueError, match="gain reference"):
        mc.refine_local_motion_raw(raw, torch.ones(4, 4), 1.0, 32)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="hot_pixel_threshold"):
            mc.refine_local_motion_raw(raw, None, 1.0, 32, hot_pixel_threshold=bad)


# ------------------------------------------------------------------ the C entry points

NEW = {"mc_xc_aligned_refs_patches": 15, "mc_xc_refine_update_patches": 13}


def test_header_and_signatures_agree_on_the_new_entry_points():
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    for name, nargs in NEW.items():
        args = header_parameters(name)
        assert len(args) == nargs == len(_lib.SIGNATURES[name])
        assert_entry_point(name, [vp if "*" in a else i32 for a in args])


def _p(i):
    return ctypes.c_void_p(0x100000 * (i + 1))


def test_entry_points_validate_on_the_host():
    """Fake pointers and a null stream: every call below must answer MC_ERR_ARG before it launches anything."""
    lib = _lib.load()

    def refs(S=_p(0), sh=_p(1), of=_p(2), fy=_p(3), fx=_p(4), G=_p(5), REF=_p(6), t=6, npatch=4, q0=0, nq=4, nkx=103,
             nky=206, under=16):
        return lib.mc_xc_aligned_refs_patches(S, sh, of, fy, fx, G, REF, t, npatch, q0, nq, nkx, nky, under, None)

    for name in ("S", "sh", "of", "fy", "fx", "G", "REF"):
        assert refs(**{name: None}) == -1, name
    assert refs(t=0) == -1 and refs(t=513) == -1 and refs(nkx=0) == -1 and refs(nky=0) == -1 and refs(under=-1) == -1
    assert refs(npatch=0) == -1 and refs(q0=-1) == -1 and refs(nq=0) == -1
    assert refs(q0=1) == -1 and refs(q0=4, nq=1) == -1  # the range leaves the patches
    assert refs(npatch=70000, nq=65536) == -1  # one grid row per patch
    assert refs(nkx=1 << 16, nky=1 << 16) == -1  # the bin index is an int

    def upd(peaks=_p(0), nb=_p(1), sh=_p(2), ref=3, t=6, npatch=4, q0=0, nq=4, H=1024, W=1024, under=16, mx=_p(3)):
        return lib.mc_xc_refine_update_patches(peaks, nb, sh, ref, t, npatch, q0, nq, H, W, under, mx, None)

    for name in ("peaks", "nb", "sh", "mx"):
        assert upd(**{name: None}) == -1, name
    assert upd(t=1) == -1 and upd(t=513) == -1 and upd(ref=-1) == -1 and upd(ref=6) == -1
    assert upd(H=1) == -1 and upd(W=1) == -1 and upd(under=-1) == -1 and upd(under=1024) == -1
    assert upd(npatch=0) == -1 and upd(q0=-1) == -1 and upd(nq=0) == -1 and upd(q0=2, nq=3) == -1
