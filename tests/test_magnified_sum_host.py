"""The aligned sum with the magnification map folded into the rigid warp (motion_correct_sum_magnified,
motion_correct_sum_magnified_raw; mc_affine_warp_sum, csrc/affine_warp_sum.hip over csrc/affine_warp_sum.h) without a
GPU: the names, the build list and the C ABI, the argument rules before any device is touched, the entry point's host
checks with fake pointers, properties of the numpy restatement (tests/magnified_sum_reference.py), and the header's
window and per-pixel bodies run on the CPU under the address and undefined-behaviour sanitizers
(tests/host_affine_warp_sum.cpp, a stand-alone program started as a child process)."""

import ctypes
import inspect
import os
import struct

import numpy as np
import pytest
import torch

import magnification_reference as mr
import magnified_sum_reference as ms
import rigid_reference as rr
from kernel_harness import assert_entry_point, run_host_program

F32 = np.float32


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


# ------------------------------------------------------------------ names, the build list, the C ABI


def test_names_parameters_and_defaults(mc):
    from torch_motion_correction_amd import magnification

    for name in ("motion_correct_sum_magnified", "motion_correct_sum_magnified_raw"):
        assert name in mc.__all__ and getattr(mc, name) is getattr(magnification, name)

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    none = inspect.Parameter.empty
    assert params(mc.motion_correct_sum_magnified) == [
        ("image", none), ("deformation_grid", none), ("pixel_spacing", none), ("major_scale", none),
        ("minor_scale", none), ("major_axis_angle", none), ("return_frames", False), ("device", None)]
    assert params(mc.motion_correct_sum_magnified_raw) == [
        ("movie", none), ("gain", none), ("deformation_grid", none), ("pixel_spacing", none), ("major_scale", none),
        ("minor_scale", none), ("major_axis_angle", none), ("mean_zero", True), ("return_frames", False),
        ("device", None)]
    for fn in (mc.motion_correct_sum_magnified, mc.motion_correct_sum_magnified_raw):
        assert "no hot-pixel step and no dose weighting" in " ".join(fn.__doc__.split())
        assert "no CPU fallback" in fn.__doc__


def test_sources_signatures_and_header_agree():
    from torch_motion_correction_amd import _build, _lib

    entry = ("affine_warp_sum.hip", "affine_warp_sum", [])
    assert _build.SOURCES[-1] != entry
    stems = [s[1] for s in _build.SOURCES]
    assert stems.index("affine_warp_sum") < stems.index("tiff_encode") < stems.index("tiff_decode") == len(stems) - 1
    for name in ("affine_warp_sum.h", "affine_resample.h"):
        assert os.path.exists(os.path.join(_build.CSRC, name))
    vp, i32, matrix = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double)  # the matrix: four host doubles
    assert_entry_point("mc_affine_warp_sum", [vp, i32, vp, vp, i32, i32, i32, matrix, vp, vp, vp, vp], source=entry)
    assert _lib.load().mc_abi_version() == 1
    rule = open(os.path.join(_build.CSRC, "affine_warp_sum.h")).read()
    assert '#include "affine_resample.h"' in rule and "hip/hip_runtime" not in rule
    assert "THE RULE" in rule and "THE SUM" in rule and "THE WINDOW" in rule


# ------------------------------------------------------------------ argument rules, before any device


def _field(t, value=1.5):
    return torch.full((2, t, 1, 1), value)


def test_argument_rules_hold_before_any_device_is_touched(mc, monkeypatch):
    from torch_motion_correction_amd import _lib, api, magnification

    def touched(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for mod in (magnification, api, _lib):
        monkeypatch.setattr(mod, "require_gpu", touched)
    for mod in (api, _lib):
        monkeypatch.setattr(mod, "device_scope", touched)
    img, movie, gain = torch.zeros(3, 5, 6), torch.zeros(3, 5, 6, dtype=torch.uint8), torch.ones(5, 6)

    def refuse(match, raw=None, **kw):
        a = dict(image=img, movie=movie, gain=gain, field=_field(3), ps=0.83, major=1.02, minor=0.98, angle=30.0)
        a.update(kw)
        tail = (a["field"], a["ps"], a["major"], a["minor"], a["angle"])
        for is_raw in ((False, True) if raw is None else (raw,)):
            with pytest.raises(ValueError, match=match):
                if is_raw:
                    mc.motion_correct_sum_magnified_raw(a["movie"], a["gain"], *tail)
                else:
                    mc.motion_correct_sum_magnified(a["image"], *tail)

    # a local field, the wrong number of time points, a field that is no (2, t, gh, gw) tensor, values that are not finite
    refuse("local field", field=torch.zeros(2, 3, 2, 2))
    refuse("local field", field=torch.zeros(2, 3, 1, 2))
    refuse("2 time points, the movie 3 frames", field=_field(2))
    for bad in (torch.zeros(3, 2), torch.zeros(3, 3, 1, 1), torch.zeros(2, 0, 1, 1), None, np.zeros((2, 3, 1, 1))):
        refuse(r"deformation_grid must be a \(2, t, 1, 1\) tensor", field=bad)
    refuse("floating-point", field=torch.zeros(2, 3, 1, 1, dtype=torch.int32))
    for bad in (float("nan"), float("inf"), -float("inf")):
        field = _field(3)
        field[1, 2, 0, 0] = bad
        refuse("deformation_grid must be finite", field=field)
    for bad in (True, float("nan"), float("inf"), None, "1.0", torch.tensor(1.0)):
        refuse("pixel_spacing must be a finite real number", ps=bad)
    for bad in (0, 0.0, -0.83):
        refuse("pixel_spacing must be > 0", ps=bad)
    refuse("overflows fp32", field=_field(3, 3e38), ps=1e-3)
    # the stack: dtype, dimensions, size
    for bad in (np.zeros((3, 5, 6), np.float32), torch.zeros(5, 6), torch.zeros(1, 3, 5, 6), torch.zeros(3, 5, 6, dtype=torch.int16),
                torch.zeros(3, 5, 6, dtype=torch.uint8), torch.zeros(3, 5, 6, dtype=torch.float64), torch.zeros(3, 5, 6, dtype=torch.bool),
                torch.zeros(3, 5, 6, dtype=torch.bfloat16), None):
        refuse(r"image must be a \(t, h, w\) tensor of dtype float32 or float16", raw=False, image=bad)
    for bad in (np.zeros((3, 5, 6), np.uint8), torch.zeros(5, 6, dtype=torch.uint8), torch.zeros(3, 5, 6), torch.zeros(3, 5, 6).half(),
                torch.zeros(3, 5, 6, dtype=torch.int32), torch.zeros(3, 5, 6, dtype=torch.int8), torch.zeros(3, 5, 6, dtype=torch.bool), None):
        refuse(r"movie must be a \(t, h, w\) tensor of dtype uint8 or int16", raw=True, movie=bad)
    refuse("image must not be empty", raw=False, image=torch.zeros(0, 5, 6), field=_field(1))
    refuse("movie must not be empty", raw=True, movie=torch.zeros(0, 5, 6, dtype=torch.int16), field=_field(1))
    for shape in ((3, 3, 6), (3, 6, 3)):
        refuse("image must have at least 4 rows and 4 columns", raw=False, image=torch.zeros(shape))
        refuse("movie must have at least 4 rows and 4 columns", raw=True, movie=torch.zeros(shape, dtype=torch.uint8),
               gain=torch.ones(shape[1:]))
    refuse("2\\^31 samples", raw=False, image=torch.zeros(1).expand(3, 1 << 16, 1 << 15))
    # the gain's shape
    for bad in (torch.ones(6, 5), torch.ones(5), torch.ones(1, 5, 6), np.ones((5, 6), np.float32)):
        refuse("gain reference has shape", raw=True, gain=bad)
    # the scales and the angle: magnification_distortion_matrix's rules, unchanged
    for name in ("major", "minor", "angle"):
        full = {"major": "major_scale", "minor": "minor_scale", "angle": "major_axis_angle"}[name]
        for bad in (True, False, float("nan"), float("inf"), None, "1.0", torch.tensor(1.0)):
            refuse(f"{full} must be a finite real number", **{name: bad})
    for name in ("major", "minor"):
        for bad in (0.8999, 1.1001, 0, -1.0, 2):
            refuse(f"{name}_scale must lie in \\[0.9, 1.1\\]", **{name: bad})
    # valid arguments get as far as the device -- the ends of the ranges, fp16, int16, no gain, float64 fields
    for image, field, ps, major, minor, angle in ((img, _field(3), 0.83, 0.9, 1.1, 0), (img.half(), _field(3).double(), 1, 1.1, 0.9, -720.5),
                                                  (img[:1], _field(1), np.float32(1.3), np.float64(1.0), 1, np.int64(30))):
        with pytest.raises(AssertionError, match="a device was touched"):
            mc.motion_correct_sum_magnified(image, field, ps, major, minor, angle, return_frames=True)
    for mv, g in ((movie, gain), (movie.to(torch.int16), None)):
        with pytest.raises(AssertionError, match="a device was touched"):
            mc.motion_correct_sum_magnified_raw(mv, g, _field(3), 0.83, 1.02, 0.98, 30.0, mean_zero=False)


def test_no_cpu_fallback(mc, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(mc.McorrError, match="no CPU fallback"):
        mc.motion_correct_sum_magnified(torch.zeros(2, 8, 8), _field(2), 0.83, 1.0, 1.0, 0.0)
    with pytest.raises(mc.McorrError, match="no CPU fallback"):
        mc.motion_correct_sum_magnified_raw(torch.zeros(2, 8, 8, dtype=torch.uint8), None, _field(2), 0.83, 1.02, 0.98, 30.0)


def test_entry_point_validates_on_the_host():
    """Fake device pointers and a null stream: every call below must answer before it touches or launches anything."""
    from torch_motion_correction_amd import _lib

    lib = _lib.load()
    ARG, UNSUPPORTED, U8, I16, F16, F32K = -1, -2, 0, 1, 2, 3
    p = {k: ctypes.c_void_p(0x10000000 * (i + 1)) for i, k in enumerate(("src", "gain", "mu", "shifts", "sum", "frames"))}
    ident = (1.0, 0.0, 0.0, 1.0)

    def call(storage=F32K, t=2, h=8, w=9, m=ident, **kw):
        a = dict(p)
        a.update(kw)
        mm = None if m is None else (ctypes.c_double * 4)(*m)
        return lib.mc_affine_warp_sum(a["src"], storage, a["gain"], a["mu"], t, h, w, mm, a["shifts"], a["sum"],
                                      a["frames"], None)

    # null pointers
    assert call(src=None) == ARG and call(shifts=None) == ARG and call(sum=None) == ARG and call(m=None) == ARG
    # sizes
    for kw in (dict(t=0), dict(t=-1), dict(h=0), dict(w=0), dict(h=-4), dict(h=3), dict(w=3), dict(h=1), dict(w=1)):
        assert call(**kw) == ARG, kw
    # storage kinds
    for storage in (-1, 4, 7):
        assert call(storage=storage) == ARG
    # gain and mu are needed for the raw kinds alone
    for storage in (U8, I16):
        assert call(storage=storage, gain=None) == ARG and call(storage=storage, mu=None) == ARG
    # a matrix affine::matrix_ok refuses
    nan, inf = float("nan"), float("inf")
    for m in ((nan, 0, 0, 1), (1, inf, 0, 1), (1, 0, -inf, 1), (1, 0, 0, nan), (0.79, 0, 0, 1), (1, 0, 0, 0.79), (1.26, 0, 0, 1),
              (1, 0, 0.2, 1.06), (0, 0, 0, 1), (1, 0, 0.5, -0.8)):
        assert call(m=m) == ARG, m
    # 2^31 samples a frame
    assert call(h=1 << 16, w=1 << 15) == UNSUPPORTED and call(storage=U8, h=1 << 15, w=1 << 16) == UNSUPPORTED
    assert call(h=1 << 16, w=1 << 15, src=None) == ARG  # the argument rules come first
    # misaligned pointers, outputs that overlap the movie or each other (2 * 8 * 9 samples)
    off = lambda q, n: ctypes.c_void_p(q.value + n)  # noqa: E731
    assert call(src=off(p["src"], 2)) == ARG and call(storage=F16, src=off(p["src"], 1)) == ARG
    assert call(sum=off(p["sum"], 2)) == ARG and call(frames=off(p["frames"], 1)) == ARG and call(shifts=off(p["shifts"], 2)) == ARG
    assert call(sum=p["src"]) == ARG and call(sum=off(p["src"], 572)) == ARG and call(frames=off(p["src"], -572)) == ARG
    assert call(frames=off(p["sum"], 284)) == ARG and call(storage=U8, sum=off(p["src"], 140)) == ARG


# ------------------------------------------------------------------ the restatement


def test_restatement_identity_and_integer_shifts_are_the_exact_sequential_sum():
    stack = mr.frames(4, 9, 11, seed=3)
    shifts = np.array([(0, 0), (2, -3), (-4, 1), (9, 0)], dtype=F32)  # the last one: wholly outside
    total, bound, vals, bnds, ins = ms.magnified_sum(stack, np.eye(2), shifts)
    shifted = ms.shifted_zero_outside(stack, shifts)
    assert np.array_equal(vals, shifted.astype(np.float64))
    assert not ins[3].any() and (vals[3] == 0).all() and (bnds[3] == 0).all()
    assert np.array_equal(ins[1], shifted[1] != 0) and int(ins[1].sum()) == 7 * 8
    want = ms.sequential_sum(shifted)
    assert want.dtype == F32 and np.array_equal(want, ((shifted[0] + shifted[1]) + shifted[2]) + shifted[3])
    # the fp32 sequence lies within the derived bound of the float64 sum, and the bound is a few ulps of the sum
    assert (np.abs(want.astype(np.float64) - total) <= bound).all()
    assert bound.max() < 1e-3 * np.abs(total).max()


def test_restatement_zero_shift_one_frame_is_the_resampler():
    frame = mr.frames(1, 40, 44, seed=5)
    zero = np.zeros((1, 2), dtype=F32)
    for params in mr.PARAMETERS:
        m = mr.matrix(*params)
        want, want_bound = mr.resample(frame[0], m, fill_value=0)
        total, bound, vals, _, ins = ms.magnified_sum(frame, m, zero)
        assert np.array_equal(total, want) and np.array_equal(vals[0], want)
        assert np.array_equal(ins[0], mr.inside_mask(40, 44, m))
        # the bound here takes each pixel's own taps, the resampler's the frame's maximum: never more, and 0 alike
        assert (bound <= want_bound).all() and np.array_equal(bound == 0, want_bound == 0)


def test_canonical_shift_keeps_the_row_the_reciprocal_shift_drops():
    """ps = 0.83, node shift -3 px: the two roundings differ there (rigid_reference.row_dropping_shifts).  Under
    identity M output row 3 samples row 3 + s: exactly 0 with the canonical shift, below 0 -- outside, zeroed -- with
    the reciprocal one."""
    ps = 0.83
    assert -3 in rr.row_dropping_shifts(rr.SMALL_SHIFTS, ps)
    field = np.zeros((2, 1, 1, 1), dtype=F32)
    field[0, 0, 0, 0] = F32(-3) * F32(ps)
    shifts = ms.pixel_shifts(field, ps)
    assert shifts.dtype == F32 and shifts.shape == (1, 2) and shifts[0, 0] == rr.canonical_shift(-3, ps) == F32(-3)
    frame = mr.frames(1, 12, 9, seed=7)
    total, _, _, _, ins = ms.magnified_sum(frame, np.eye(2), shifts)
    assert ins[0, 3].all() and not ins[0, :3].any() and np.array_equal(total[3], frame[0, 0].astype(np.float64))
    bad = np.array([[rr.reciprocal_shift(-3, ps), 0]], dtype=F32)
    assert bad[0, 0] < -3
    total, _, _, _, ins = ms.magnified_sum(frame, np.eye(2), bad)
    assert not ins[0, 3].any() and (total[3] == 0).all()
    # and the package's own division is the canonical one
    from torch_motion_correction_amd import magnification

    for s in rr.SMALL_SHIFTS:
        f = torch.zeros(2, 1, 1, 1)
        f[:, 0, 0, 0] = torch.tensor(np.float32(s) * np.float32(ps))
        got = magnification._pixel_shifts(f, 1, ps)
        assert got.dtype == torch.float32 and got.shape == (1, 2) and got.device.type == "cpu"
        assert float(got[0, 0]) == float(got[0, 1]) == float(rr.canonical_shift(s, ps))


# ------------------------------------------------------------------ the header's bodies on the CPU, sanitized


def _cases():
    """-> [(stack fp32, M, shifts fp32 (t, 2))]: the extreme matrices, shifts of +-0.5, +-150.25 and one larger than
    any frame, every shape; identity M with whole-pixel shifts; a movie whose every frame lies wholly outside."""
    out = []
    shifts = np.array([(0.5, -0.5), (-0.5, 0.5), (0.0, 150.25), (0.5, -150.25), (150.25, 0.0), (-150.25, -0.5),
                       (2000.0, -2000.0)], dtype=F32)
    for h, w in ((4, 4), (61, 67), (130, 257)):
        for params in ((1.1, 0.9, 45.0), (0.9, 0.9, 0.0), (1.02, 0.98, 30.0)):
            out.append((mr.frames(len(shifts), h, w, seed=11), mr.matrix(*params), shifts))
        whole = np.array([(0, 0), (3, -2), (-70, 5), (1, 66), (-200, 0)], dtype=F32)
        out.append((mr.frames(len(whole), h, w, seed=12), np.eye(2), whole))
        far = np.array([(1e4, 0.0), (0.0, -1e4), (-3e38, 3e38)], dtype=F32)
        out.append((mr.frames(len(far), h, w, seed=13), mr.matrix(1.1, 0.9, 45.0), far))
    return out


def test_bodies_on_the_host_under_sanitizers(tmp_path):
    """csrc/affine_warp_sum.h -- the window rule and the per-pixel body affine_warp_sum.hip compiles for the device --
    built for the host with -fsanitize=address,undefined into a program of its own and run as a child process: sums
    made tile after tile and frame after frame on a movie and a window (rows x STRIDE floats) allocated to their exact
    sizes, so that a stray read is a sanitizer report and a window beyond WIN = 83 a failure.  Positions and inside
    masks are compared with the restatement bit for bit, the sums within the derived bound; identity M with
    whole-pixel shifts bit for bit with the fp32 sequential sum; a movie shifted wholly outside sums to exact zeros
    with every (tile, frame) skipped.  Nothing sanitized is loaded into this process."""
    cases = _cases()
    blob = b"".join(struct.pack("<4i4d", *stack.shape, 0, *np.asarray(m, dtype=np.float64).ravel())
                    + shifts.astype("<f4").tobytes() + stack.astype("<f4").tobytes() for stack, m, shifts in cases)
    (tmp_path / "cases.bin").write_bytes(blob)
    res = run_host_program("host_affine_warp_sum.cpp", tmp_path, tmp_path / "cases.bin", tmp_path / "results.bin")
    assert f"{len(cases)} cases, 0 failures" in res.stdout
    raw = (tmp_path / "results.bin").read_bytes()
    pos = 0
    for i, (stack, m, shifts) in enumerate(cases):
        t, h, w = stack.shape
        n = h * w
        got = np.frombuffer(raw, "<f4", n, pos).reshape(h, w)
        pos += 4 * n
        total, bound, vals, _, ins = ms.magnified_sum(stack, m, shifts)
        for f in range(t):
            py = np.frombuffer(raw, "<f8", n, pos).reshape(h, w)
            px = np.frombuffer(raw, "<f8", n, pos + 8 * n).reshape(h, w)
            inside = np.frombuffer(raw, np.uint8, n, pos + 16 * n).reshape(h, w)
            pos += 17 * n
            wpy, wpx = ms.positions(h, w, m, shifts[f, 0], shifts[f, 1])
            assert np.array_equal(py.view(np.int64), wpy.view(np.int64)), (i, f)
            assert np.array_equal(px.view(np.int64), wpx.view(np.int64)), (i, f)
            assert np.array_equal(inside.astype(bool), ins[f]), (i, f)
        err = np.abs(got.astype(np.float64) - total)
        assert (err <= bound).all(), (i, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.array_equal(got[bound == 0], np.zeros(int((bound == 0).sum()), F32))
        if np.array_equal(m, np.eye(2)):
            want = ms.sequential_sum(ms.shifted_zero_outside(stack, shifts))
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), i
        if not ins.any():
            assert not got.any() and f"case {i} " in res.stdout
            tiles = ((h + 63) // 64) * ((w + 63) // 64)
            assert f"{tiles * t} tile-frames skipped" in [ln for ln in res.stdout.splitlines() if ln.startswith(f"case {i} ")][0]
    assert pos == len(raw)
    # the general cases do sample: some frames inside, some tiles skipped, no window beyond the bound
    assert any("0 tile-frames skipped" not in ln for ln in res.stdout.splitlines() if ln.startswith("case "))
