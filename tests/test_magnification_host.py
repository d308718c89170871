"""Magnification distortion correction (magnification_distortion_matrix, correct_magnification_distortion;
mc_affine_resample, csrc/affine_resample.hip over csrc/affine_resample.h) without a GPU: the names, the build list and
the C ABI, the matrix and its convention, the argument rules before any device is touched, the entry point's host
checks with fake pointers, the numpy restatement (tests/magnification_reference.py) against grid_sample in float64,
the GPU tests' cases checked for knife-edge positions, and the header's window and per-pixel bodies run on the CPU
under the address and undefined-behaviour sanitizers (tests/host_affine_resample.cpp, a stand-alone program started as
a child process)."""

import ctypes
import inspect
import os
import re
import struct

import numpy as np
import pytest
import torch

import magnification_reference as mr
from kernel_harness import assert_entry_point, header_parameters, run_host_program



@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


# ------------------------------------------------------------------ names, the build list, the C ABI


def test_names_parameters_and_defaults(mc):
    from torch_motion_correction_amd import magnification

    for name in ("magnification_distortion_matrix", "correct_magnification_distortion"):
        assert name in mc.__all__ and getattr(mc, name) is getattr(magnification, name)

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    none = inspect.Parameter.empty
    assert params(mc.magnification_distortion_matrix) == [("major_scale", none), ("minor_scale", none),
                                                          ("major_axis_angle", none)]
    assert params(mc.correct_magnification_distortion) == [("image", none), ("major_scale", none), ("minor_scale", none),
                                                           ("major_axis_angle", none), ("fill_value", 0.0),
                                                           ("device", None)]
    assert "own" in mc.correct_magnification_distortion.__doc__ and "not" in mc.magnification_distortion_matrix.__doc__


def test_sources_signatures_and_header_agree():
    from torch_motion_correction_amd import _build

    vp, i32 = ctypes.c_void_p, ctypes.c_int
    assert_entry_point("mc_affine_resample",
                       [vp, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_double), ctypes.c_float, vp, vp],
                       source=("affine_resample.hip", "affine_resample", []))
    assert os.path.exists(os.path.join(_build.CSRC, "affine_resample.h"))
    args = header_parameters("mc_affine_resample")
    kinds = ["*" if "*" in a else a.split()[0] for a in args]
    assert kinds == ["*", "int", "int", "int", "int", "const", "float", "*", "*"] and "const double m[4]" in args
    rule = open(os.path.join(_build.CSRC, "affine_resample.h")).read()
    assert "hip/hip_runtime" not in rule and "THE RULE" in rule and "ACCUMULATION" in rule
    # the header's window bound, restated: floor(1.25 * (TILE - 1)) + 1 + 4 rows of STRIDE floats, in 64 KiB of LDS
    tile = int(re.search(r"constexpr int TILE = (\d+);", rule).group(1))
    stride = int(re.search(r"constexpr int STRIDE = (\d+);", rule).group(1))
    win = int(1.25 * (tile - 1)) + 1 + 4
    assert f"WIN == {win}" in rule and stride >= win and stride % 32 == 0 and win * stride * 4 <= 65536


# ------------------------------------------------------------------ the matrix and its convention


def test_matrix_is_d_in_yx_order(mc):
    for major, minor, angle in mr.PARAMETERS + ((1.05, 0.93, -72.5), (0.95, 1.08, 200.0)):
        m = mc.magnification_distortion_matrix(major, minor, angle)
        assert m.dtype == torch.float64 and m.shape == (2, 2) and m.device.type == "cpu"
        m = m.numpy()
        assert np.abs(m - mr.matrix(major, minor, angle)).max() <= 1e-15
        d = m[::-1, ::-1]  # (x, y) order
        assert d[0, 1] == d[1, 0]  # symmetric
        assert np.allclose(np.sort(np.linalg.eigvalsh(d)), sorted((major, minor)), rtol=0, atol=1e-14)
        a = np.deg2rad(angle)
        u = np.array([np.cos(a), np.sin(a)])
        assert np.allclose(d @ u, major * u, rtol=0, atol=1e-14)  # the major axis is an eigenvector of `major`
        assert np.allclose(d @ np.array([-u[1], u[0]]), minor * np.array([-u[1], u[0]]), rtol=0, atol=1e-14)


def test_matrix_symmetries(mc):
    f = mc.magnification_distortion_matrix
    for major, minor, angle in mr.PARAMETERS + ((1.05, 0.93, -72.5), (0.95, 1.08, 100.0)):
        m = f(major, minor, angle)
        assert (f(major, minor, angle + 180.0) - m).abs().max() <= 1e-15
        assert (f(major, minor, angle - 180.0) - m).abs().max() <= 1e-15
        assert (f(minor, major, angle + 90.0) - m).abs().max() <= 1e-15


def test_matrix_hand_computed_cases(mc):
    f = mc.magnification_distortion_matrix
    # angle 0: the major axis is x (columns): M[1, 1] carries it, rows are untouched
    assert (f(1.05, 1.0, 0.0) - torch.tensor([[1.0, 0.0], [0.0, 1.05]], dtype=torch.float64)).abs().max() <= 1e-15
    assert f(1.05, 1.0, 0.0)[0, 1] == 0 and f(1.05, 1.0, 0.0)[1, 0] == 0
    # angle 90: the major axis is y (rows)
    assert (f(1.05, 1.0, 90.0) - torch.tensor([[1.05, 0.0], [0.0, 1.0]], dtype=torch.float64)).abs().max() <= 1e-15
    # angle 45: D = [[1.025, 0.025], [0.025, 1.025]]; the off-diagonal is positive (from +x TOWARDS +y)
    assert (f(1.05, 1.0, 45.0) - torch.tensor([[1.025, 0.025], [0.025, 1.025]], dtype=torch.float64)).abs().max() <= 1e-15
    assert f(1.05, 1.0, 135.0)[0, 1] < 0
    # equal scales: exactly that multiple of the identity, whatever the angle; 1, 1 is exactly the identity
    assert torch.equal(f(1, 1, 33.0), torch.eye(2, dtype=torch.float64))
    assert torch.equal(f(1.1, 1.1, 45.0), 1.1 * torch.eye(2, dtype=torch.float64))
    # the positions of the hand case: x stretched about the centre column, y untouched
    py, px = mr.positions(6, 9, f(1.05, 1.0, 0.0).numpy())
    assert np.array_equal(py, np.broadcast_to(np.arange(6.0)[:, None], (6, 9)))
    assert np.allclose(px, np.broadcast_to(4 + 1.05 * (np.arange(9.0) - 4)[None, :], (6, 9)), rtol=0, atol=1e-14)


# ------------------------------------------------------------------ argument rules, before any device


def test_argument_rules_hold_before_any_device_is_touched(mc, monkeypatch):
    from torch_motion_correction_amd import _lib, api, magnification

    def touched(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    for mod in (magnification, api, _lib):
        monkeypatch.setattr(mod, "require_gpu", touched)
    monkeypatch.setattr(api, "device_scope", touched)
    img = torch.zeros(2, 5, 6)

    def refuse(match, image=img, major=1.02, minor=0.98, angle=30.0, **kw):
        with pytest.raises(ValueError, match=match):
            mc.correct_magnification_distortion(image, major, minor, angle, **kw)

    for bad in (np.zeros((5, 6), np.float32), torch.zeros(5), torch.zeros(1, 2, 5, 6), torch.zeros(5, 6, dtype=torch.int16),
                torch.zeros(2, 5, 6, dtype=torch.uint8), torch.zeros(5, 6, dtype=torch.int32), torch.zeros(5, 6, dtype=torch.bool),
                torch.zeros(5, 6, dtype=torch.float64), torch.zeros(5, 6, dtype=torch.bfloat16), None, [[1.0] * 4] * 4):
        refuse(r"image must be an \(h, w\) or \(t, h, w\) tensor of dtype float32 or float16", image=bad)
    refuse("image must not be empty", image=torch.zeros(0, 5, 6))
    for bad in (torch.zeros(3, 6), torch.zeros(2, 6, 3), torch.zeros(4, 3, dtype=torch.float16)):
        refuse("image must have at least 4 rows and 4 columns", image=bad)
    refuse("2\\^31 samples", image=torch.zeros(1).expand(1, 1 << 16, 1 << 15))
    for name in ("major", "minor", "angle"):
        full = {"major": "major_scale", "minor": "minor_scale", "angle": "major_axis_angle"}[name]
        for bad in (True, False, float("nan"), float("inf"), -float("inf"), None, "1.0", [1.0], torch.tensor(1.0), 1 + 0j):
            refuse(f"{full} must be a finite real number", **{name: bad})
            with pytest.raises(ValueError, match=f"{full} must be a finite real number"):
                mc.magnification_distortion_matrix(**{"major_scale": 1.0, "minor_scale": 1.0, "major_axis_angle": 0.0,
                                                      full: bad})
    for name in ("major", "minor"):
        for bad in (0.8999, 1.1001, 0, -1.0, 2):
            refuse(f"{name}_scale must lie in \\[0.9, 1.1\\]", **{name: bad})
    for bad in (True, float("nan"), float("inf"), None, "0", torch.tensor(0.0)):
        refuse("fill_value must be a finite real number", fill_value=bad)
    # the ends of the range, integers and numpy scalars are taken; valid arguments get as far as the device
    for image, major, minor, angle, fill in ((img, 0.9, 1.1, 0, 0.0), (img[0], 1.1, 0.9, -720.5, -3.5), (img.half(), 1, 1, 0.0, 1),
                                             (img, np.float64(1.02), np.float32(1.0), np.int64(30), np.float32(2.0))):
        with pytest.raises(AssertionError, match="a device was touched"):
            mc.correct_magnification_distortion(image, major, minor, angle, fill_value=fill)


def test_no_cpu_fallback(mc, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(mc.McorrError, match="no CPU fallback"):
        mc.correct_magnification_distortion(torch.zeros(8, 8), 1.0, 1.0, 0.0)


def test_entry_point_validates_on_the_host():
    """Fake device pointers and a null stream: every call below must answer before it touches or launches anything."""
    from torch_motion_correction_amd import _lib

    lib = _lib.load()
    ARG, UNSUPPORTED, F16, F32 = -1, -2, 2, 3
    src, dst = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x20000000)
    ident = (1.0, 0.0, 0.0, 1.0)

    def call(src=src, storage=F32, n=2, h=8, w=9, m=ident, fill=0.0, dst=dst):
        mm = None if m is None else (ctypes.c_double * 4)(*m)
        return lib.mc_affine_resample(src, storage, n, h, w, mm, fill, dst, None)

    assert call(src=None) == ARG and call(dst=None) == ARG and call(m=None) == ARG
    assert call(n=0) == ARG and call(n=-1) == ARG and call(h=3) == ARG and call(w=3) == ARG and call(h=0) == ARG
    for storage in (0, 1, 4, -1):
        assert call(storage=storage) == UNSUPPORTED
    assert call(storage=0, n=0) == ARG  # the sizes come before the storage
    assert call(h=1 << 16, w=1 << 15) == UNSUPPORTED  # 2^31 samples a frame
    nan, inf = float("nan"), float("inf")
    for m in ((nan, 0, 0, 1), (1, inf, 0, 1), (1, 0, -inf, 1), (1, 0, 0, nan)):
        assert call(m=m) == ARG, m
    # row sums of |entries| outside [0.8, 1.25]
    for m in ((0.79, 0, 0, 1), (1, 0, 0, 0.79), (1.26, 0, 0, 1), (1, 0, 0.2, 1.06), (0.7, -0.56, 0, 1), (0, 0, 0, 1),
              (1, 0, 0.5, -0.8), (-0.4, 0.39, 0, 1)):
        assert call(m=m) == ARG, m
    # dst must not alias src: equal, and byte ranges that overlap (2 * 8 * 9 samples: 576 bytes fp32, 288 fp16)
    assert call(dst=src) == ARG
    assert call(dst=ctypes.c_void_p(src.value + 572)) == ARG and call(dst=ctypes.c_void_p(src.value - 572)) == ARG
    assert call(storage=F16, dst=ctypes.c_void_p(src.value + 284)) == ARG
    assert call(src=ctypes.c_void_p(src.value + 2)) == ARG and call(dst=ctypes.c_void_p(dst.value + 2)) == ARG
    assert call(storage=F16, src=ctypes.c_void_p(src.value + 1)) == ARG


# ------------------------------------------------------------------ the restatement


def test_restatement_identity_and_fill():
    img = mr.frames(2, 9, 11)
    out, bound = mr.resample(img, np.eye(2), fill_value=7.0)
    assert np.array_equal(out, img.astype(np.float64)) and (bound > 0).all()
    # scale 1.1 about the centre (4, 5) of a 9 x 11 frame: rows 4 +- 1.1 k leave [0, 8] for |k| = 4
    out, bound = mr.resample(img[0], 1.1 * np.eye(2), fill_value=-3.5)
    inside = mr.inside_mask(9, 11, 1.1 * np.eye(2))
    want = np.zeros((9, 11), bool)
    want[1:8, 1:10] = True  # columns 5 +- 1.1 k: |k| <= 4 stay inside [0, 10]
    assert np.array_equal(inside, want) and (out[~inside] == -3.5).all() and (bound[~inside] == 0).all()
    assert out[4, 5] == img[0, 4, 5]  # the centre maps to itself
    # the bound per unit of max |image|: 2 * 51.6 u + 8 u at fractions of 0 (the derivation's own sums), below 200 u
    t = np.linspace(0, 1, 33).astype(np.float32)
    factor = mr.bound_factor(*np.broadcast_arrays(t[:, None], t[None, :]))
    assert factor.shape == (33, 33) and factor[0, 0] == pytest.approx(111.2 * mr.U, rel=1e-3)
    assert 100 * mr.U < factor.min() and factor.max() < 200 * mr.U


def test_restatement_against_grid_sample_float64():
    """The restatement against torch's grid_sample (bicubic, border padding, align_corners=True) in FLOAT64 on the CPU,
    for an interior crop of a 40 x 44 image: an independent evaluation of the same positions, taps and Keys weights.
    It does not round the fractions to fp32, which the bound allows for: the tolerance is the fp32 bound itself."""
    h, w = 40, 44
    img = mr.frames(1, h, w, seed=5)[0]
    for major, minor, angle in mr.PARAMETERS:
        m = mr.matrix(major, minor, angle)
        want, bound = mr.resample(img, m)
        py, px = mr.positions(h, w, m)
        grid = torch.from_numpy(np.stack([2 * px / (w - 1) - 1, 2 * py / (h - 1) - 1], axis=-1))[None]
        got = torch.nn.functional.grid_sample(torch.from_numpy(img.astype(np.float64))[None, None], grid, mode="bicubic",
                                              padding_mode="border", align_corners=True)[0, 0].numpy()
        crop = (slice(8, h - 8), slice(8, w - 8))
        assert mr.inside_mask(h, w, m)[crop].all()
        err = np.abs(got - want)[crop]
        assert (err <= bound[crop]).all(), (major, minor, angle, float((err / bound[crop]).max()))
        assert np.abs(want[crop] - img[crop]).max() > 0.1  # and the resampling does something


def test_gpu_cases_have_no_knife_edge_positions(mc):
    """No source position of the GPU tests' cases lies within 1e-9 of 0, h - 1 or w - 1: the inside / outside decision
    never hinges on one float64 ulp.  The identity's positions are exact integers and are not among these cases.

    ONE combination cannot be moved off the edge by changing the angle, because an isotropic scale has no angle: 1.1 on
    67 columns puts column 3 at px = 33 + fl(1.1 * -30) (and column 63 at 33 + fl(1.1 * 30), against w - 1 = 66), and
    1.1 * 30 is 33 in the reals.  The rule evaluates the
    product and the sum separately (csrc/affine_resample.h): the double 1.1 times 30 is 33 + 2.7e-15, which rounds to
    33, so px is exactly 0.0 (66.0) and the pixel is INSIDE; a fused multiply-add would give -2.7e-15 and fill_value.  The
    case stays in the GPU test as the issue sets it, with every pixel compared: there it pins the unfused evaluation.
    Here: those are the only positions near an edge, and they are exactly on it."""
    for _, h, w in mr.SHAPES:
        for major, minor, angle in mr.PARAMETERS:
            m = mc.magnification_distortion_matrix(major, minor, angle).numpy()  # what the GPU tests resample through
            if (h, w, major, minor) == (61, 67, 1.1, 1.1):
                assert np.array_equal(m, 1.1 * np.eye(2))
                py, px = mr.positions(h, w, m)
                assert (px[:, 3] == 0.0).all() and (px[:, 63] == 66.0).all()
                assert mr.inside_mask(h, w, m)[3:58, 3].all() and mr.inside_mask(h, w, m)[3:58, 63].all()
                assert 33.0 + np.float64(1.1) * -30.0 == 0.0 and float(np.float64(1.1)).hex() == "0x1.199999999999ap+0"
                px[:, (3, 63)] = 1.0  # every other position keeps the margin
                assert min(np.abs(py).min(), np.abs(py - 60).min(), np.abs(px).min(), np.abs(px - 66).min()) > 1e-3
                continue
            assert mr.edge_distance(h, w, m) > mr.EDGE_MARGIN, (h, w, major, minor, angle)
    assert mr.edge_distance(61, 67, np.eye(2)) == 0.0


# ------------------------------------------------------------------ the header's bodies on the CPU, sanitized


def _record(frame, m, fill):
    h, w = frame.shape
    want, bound = mr.resample(frame, m, fill)
    return struct.pack("<iifi4d", h, w, fill, 0, *np.asarray(m, dtype=np.float64).ravel()) + frame.astype("<f4").tobytes() \
        + want.astype("<f8").tobytes() + bound.astype("<f8").tobytes()


def test_bodies_on_the_host_under_sanitizers(tmp_path):
    """csrc/affine_resample.h -- the window rule and the per-pixel body affine_resample.hip compiles for the device --
    built for the host with -fsanitize=address,undefined into a program of its own and run as a child process over
    whole frames of 4 x 4, 5 x 7 and 33 x 65 with the scales at both ends of their range (every clamp and the fill
    branch), and over frames of several tiles with matrices at the entry point's own bounds (row sums of 0.8 and 1.25,
    quarter turns and reflections among them: the largest windows).  Frame and window are allocated to their exact
    sizes: a stray read is a sanitizer report.  The output is compared with the restatement's within its bound, the
    filled pixels bit for bit.  Nothing sanitized is loaded into this process."""
    records, fills = [], (0.0, -3.5)
    scales = ((0.9, 0.9, 0.0), (1.1, 1.1, 0.0), (0.9, 1.1, 30.0), (1.1, 0.9, 117.0), (1.0, 1.0, 0.0), (1.1, 1.1, 45.0))
    for h, w in ((4, 4), (5, 7), (33, 65)):
        frame = mr.frames(1, h, w, seed=1)[0]
        for i, (major, minor, angle) in enumerate(scales):
            m = mr.matrix(major, minor, angle)
            if (major, minor) == (1.0, 1.0):
                m = np.eye(2)
            records.append(_record(frame, m, fills[i % 2]))
            if (major, minor) == (1.1, 1.1):
                assert not mr.inside_mask(h, w, m).all()  # the fill branch runs
    bounds = ([[0.0, -1.25], [1.25, 0.0]], [[0.0, 1.25], [-1.25, 0.0]], [[-1.25, 0.0], [0.0, 1.25]], [[0.8, 0.0], [0.0, -0.8]],
              [[0.625, 0.625], [-0.625, 0.625]], [[1.0, -0.25], [0.25, 1.0]], [[0.4, 0.4], [0.8, 0.0]])
    for h, w in ((130, 150), (70, 200)):
        frame = mr.frames(1, h, w, seed=2)[0]
        for m in bounds:
            records.append(_record(frame, np.array(m), 1.5))
    cases = tmp_path / "cases.bin"
    cases.write_bytes(b"".join(records))
    res = run_host_program("host_affine_resample.cpp", tmp_path, cases)
    assert f"{len(records)} cases, 0 failures" in res.stdout
