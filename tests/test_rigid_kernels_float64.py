"""Every rigid-warp kernel (csrc/warp_rigid.hip: warp_rigid_dma, warp_rigid, warp_rigid_dma_h;
csrc/warp_rigid_raw.hip: warp_rigid_raw) against the float64 gather resampler of tests/rigid_reference.py at FRACTIONAL shifts, on frames of one to 1024 tiles, with
no knife-edge mask and no excluded pixel (the share of pixels left out is 0).

The kernels are driven through the C ABI (mc_warp_rigid_phase_t, mc_warp_rigid_raw, mc_warp_rigid_raw_accumulate)
with the test's own (t, 2) fp32 `shifts_px`: nothing here depends on fields, lattices or the pixel spacing (those
routes are pinned by tests/test_rigid_routes.py).  Every case runs the three output combinations -- frames only
(the frames_in_grid = 1 grid), sum only, frames + sum -- into NaN-filled buffers with NaN guard words around them.

Bounds (none is fitted to a kernel's output; the reference is the only thing a tolerance is measured against):

  frames  |got - ref| <= 32 * 2^-24 * mag + wterm per pixel.
          mag = sum_ij |wy_i| |wx_j| |v_ij| over the 16 taps as the kernels evaluate them; 32 * 2^-24 * mag is the
          fp32 term of test_rigid_routes._frame_bound (two cubic weights per product at <= 8 ulp each, and the
          separable 4 + 4-term sums).  The rigid kernels use the reference's own fp32 coordinate chain, so there is
          no coordinate term.
          wterm: on the GPU that term ALONE proved too tight at fractional shifts, for a reason with a name: the
          8 ulp per weight hold for weights near 1 only.  The Horner forms of the cubic weights (ATen's, which
          cubic_coeffs_fast evaluates) cancel from intermediates of magnitude 3 to 6 down to |w| <= 0.15 for the
          far taps -- to 2e-4 at a fraction of 2^-12 -- so a weight's fp32 error is ABSOLUTE, up to 27 * 2^-24 for
          a far tap and 6.2 * 2^-24 for a near one (rigid_reference.cubic_weight_error: the derivation, rounding by
          rounding; an operation-by-operation fp32 evaluation on the host reaches 20 * 2^-24,
          test_cubic_weight_error_bounds_an_fp32_evaluation).  With the 32-ulp term alone 28 of these 37 tests
          failed, worst |got - ref| / bound = 20 at the shift (3 + 2^-12, -12 + 2^-11) of warp_rigid_dma
          (3, 33, 516), at a pixel whose main tap is 0.004 among neighbours of 5.  The bound is therefore widened by
          exactly that named amount, wterm = sum_ij ((|wy_i| + ey_i) (|wx_j| + ex_j) - |wy_i| |wx_j|) |v_ij| with
          e = cubic_weight_error of the tap; the constant 32 stays.
          The fp16 kernel gets the same bound on the up-cast values (the widening is exact).
  raw     the conditioning c = raw * gain - mu in fp32 is at most two roundings of magnitudes <= |raw * gain| +
          |mu| (raw, gain and mu are exact fp32 values): |c - v| <= 2 * 2^-24 * (|raw * gain| + |mu|) per sample
          against v = float64(raw) * float64(gain) - float64(mu) (mu = the kernel's own fp32 means,
          engine.RawMovie.mu).  A sample error e_ij reaches the output as sum_ij wy_i wx_j e_ij, at most
          sum_ij |wy_i| |wx_j| |e_ij|: the error map resampled with the absolute weights (the magnitude pass) is
          added to the frame bound.
  sum     |sum - ref.sum(0)| <= sum_f bound_f + t * 2^-24 * sum_f |ref_f| (test_rigid_routes' sum_bound: the t - 1
          adds of the register accumulator); mc_warp_rigid_raw_accumulate adds one fp32 add per pixel and chunk.
  zeros   the kernel's frames are zero exactly where the reference's are (inputs have no zero sample; for raw
          movies the reference asserts that no conditioned sample is exactly zero).

Measured worst |got - ref| / bound over all cases of a kernel, from one run on an MI355X (frames / sum) -- the
headroom for whoever next rewrites the strip body:

  warp_rigid_dma (fp32, also the unaligned sum)        0.135 / 0.129   ((2, 4096, 4096): 0.082 / 0.081)
  warp_rigid (register tile, also offset pointers)     0.171 / 0.132
  warp_rigid_dma_h (fp16)                              0.132 / 0.106
  warp_rigid_raw u8 (also t = 256, re-centring)        0.241 / 0.205
  warp_rigid_raw i16                                   0.268 / 0.209
  mc_warp_rigid_raw_accumulate                         -     / 0.221
  motion_correct_sum_raw at t = 257 (fp32 fallback)    0.222 / 0.029
"""

import ctypes as C

import numpy as np
import pytest
import torch

from kernel_harness import (assert_guards, assert_sum, float_stack, lib, mc, nan_buffer, offset_copy,  # noqa: F401
                            raw_setup)
from rigid_reference import (KERNEL_CASES, RECENTRE_SHIFTS, assert_frames, condition_float64, conditioning_error,
                             kernel_case_shifts, rigid_resample_gather_stack)

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
MODES = ("frames", "sum", "frames+sum")


# ------------------------------------------------------------------ buffers and launches


def _scratch(lib, t, h, w, dev):
    from torch_motion_correction_amd._lib import check

    nbytes = C.c_int64(0)
    check(lib.mc_warp_rigid_scratch_bytes(t, h, w, C.byref(nbytes)), "mc_warp_rigid_scratch_bytes")
    return torch.zeros((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)


def _float_launcher(lib, src):
    """launch(shifts, scratch, frames, total, phase) of mc_warp_rigid_phase_t over the fp32 / fp16 stack `src`."""
    from torch_motion_correction_amd import engine
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    t, h, w = src.shape
    storage = engine.storage_of(src)

    def launch(shifts, scratch, frames, total, phase):
        check(lib.mc_warp_rigid_phase_t(ptr(src), storage, t, h, w, ptr(shifts), ptr(scratch), ptr(frames),
                                        ptr(total), phase, stream_ptr(src.device)), "mc_warp_rigid_phase_t")

    return launch


def _raw_launcher(lib, rm, accumulate=False):
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    t, h, w = rm.shape
    entry = lib.mc_warp_rigid_raw_accumulate if accumulate else lib.mc_warp_rigid_raw

    def launch(shifts, scratch, frames, total, phase):
        check(entry(ptr(rm.raw), rm.kind, ptr(rm.gain), ptr(rm.mu), t, h, w, ptr(shifts), ptr(scratch), ptr(frames),
                    ptr(total), phase, stream_ptr(rm.raw.device)), "mc_warp_rigid_raw")

    return launch


# ------------------------------------------------------------------ references


def _float_reference(src):
    """shifts (t, 2) -> (ref, frame bound) of an fp32 / fp16 stack (a CPU tensor), both (t, h, w) float64."""
    values = src.float().numpy()
    assert not (values == 0).any()

    def reference(shifts):
        ref, mag, wterm = rigid_resample_gather_stack(lambda f: values[f], shifts, weight_error=True)
        return ref, 32 * ULP * mag + wterm

    return reference


def _raw_reference(raw, gain, mu):
    """The same for a raw movie (CPU tensors; gain None = ones; mu the kernel's fp32 frame means): the float64
    conditioning, and the conditioning rounding propagated through the absolute weights added to the bound."""
    raw_np = raw.numpy()
    gain_np = None if gain is None else gain.numpy()
    mu_np = np.asarray(mu, dtype=np.float32)

    def frame(f):
        v = condition_float64(raw_np[f], gain_np, mu_np[f])
        assert not (v == 0).any(), "a conditioned sample is exactly zero: pick another gain / movie"
        return v

    def reference(shifts):
        ref, mag, err, wterm = rigid_resample_gather_stack(
            frame, shifts, extra=lambda f: conditioning_error(raw_np[f], gain_np, mu_np[f]), weight_error=True)
        return ref, 32 * ULP * mag + wterm + err

    return reference


def _sum_bound(ref, bound):
    return bound.sum(0) + ref.shape[0] * ULP * np.abs(ref).sum(0)


def _run_case(lib, launch, reference, shape, shifts, dev, what, frames_offset=0, sum_offset=0, modes=MODES):
    """Every chunk of t shifts x every output combination against the reference (computed once per chunk).
    Returns the worst |got - ref| / bound of the frames and of the sums."""
    t, h, w = shape
    scratch = _scratch(lib, t, h, w, dev)
    worst_f = worst_s = 0.0
    for a in range(0, len(shifts), t):
        chunk = np.ascontiguousarray(shifts[a:a + t], dtype=np.float32)
        sd = torch.from_numpy(chunk).to(dev)
        ref, bound = reference(chunk)
        sum_bound = _sum_bound(ref, bound)
        for mode in modes:
            tag = f"{what} shifts {chunk.tolist()} [{mode}]"
            frames, frames_all = nan_buffer((t, h, w), dev, frames_offset) if "frames" in mode else (None, None)
            total, total_all = nan_buffer((h, w), dev, sum_offset) if "sum" in mode else (None, None)
            launch(sd, scratch, frames, total, 0)
            torch.cuda.synchronize()
            if frames is not None:
                assert_guards(frames, frames_all, tag)
                worst_f = max(worst_f, assert_frames(frames, ref, bound, tag))
            if total is not None:
                assert_guards(total, total_all, tag)
                worst_s = max(worst_s, assert_sum(total, ref.sum(0), sum_bound, tag))
            del frames, frames_all, total, total_all
    print(f"RATIO {what}: frames {worst_f:.3f} sum {worst_s:.3f}")
    return worst_f, worst_s


def _assert_phases_split(lib, launch, shape, shifts, dev, what):
    """Phase 1 (tables) + phase 2 (resampling) give the bits of phase 0."""
    t, h, w = shape
    sd = torch.from_numpy(np.ascontiguousarray(shifts[:t], dtype=np.float32)).to(dev)
    out = []
    for phases in ((0,), (1, 2)):
        scratch = _scratch(lib, t, h, w, dev)
        frames, _ = nan_buffer((t, h, w), dev)
        total, _ = nan_buffer((h, w), dev)
        for ph in phases:
            launch(sd, scratch, None if ph == 1 else frames, None if ph == 1 else total, ph)
        torch.cuda.synchronize()
        out.append((frames, total))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), what
    assert not bool(torch.isnan(out[0][0]).any()) and not bool(torch.isnan(out[0][1]).any()), what


def _case_id(case):
    return "x".join(str(v) for v in case[:3])


# ------------------------------------------------------------------ fp32: warp_rigid_dma


@pytest.mark.parametrize("case", KERNEL_CASES["warp_rigid_dma"], ids=_case_id)
def test_warp_rigid_dma_matches_the_float64_resampler(lib, dev, case):
    """w % 4 == 0, aligned buffers: the LDS-DMA kernel.  (3, 33, 516): the last tile has one row and one quad;
    (3, 32, 512): exactly one full tile; (3, 64, 2048): 8 tiles, the XCD band remap with full tiles; (3, 96, 1536):
    9 tiles, no remap; (2, 4096, 4096): the benchmark geometry, 1024 tiles (with fractional
    shifts).  The first case also runs the phase 1 + phase 2 split."""
    t, h, w = case[:3]
    src = float_stack(t, h, w)
    launch = _float_launcher(lib, src.to(dev))
    shifts = kernel_case_shifts(*case)
    _run_case(lib, launch, _float_reference(src), (t, h, w), shifts, dev, f"warp_rigid_dma {(t, h, w)}")
    if case == KERNEL_CASES["warp_rigid_dma"][0]:
        _assert_phases_split(lib, launch, (t, h, w), shifts, dev, "warp_rigid_dma phases")


@pytest.mark.parametrize("case", [KERNEL_CASES["warp_rigid_dma"][3], KERNEL_CASES["warp_rigid_dma"][0]], ids=_case_id)
def test_warp_rigid_dma_unaligned_sum(lib, dev, case):
    """`out_sum` 4 bytes past a 16-byte boundary of a larger buffer, frames aligned: the scalar-store branch of the
    sum (full tiles, and a last tile of one row and one quad)."""
    t, h, w = case[:3]
    src = float_stack(t, h, w)
    _run_case(lib, _float_launcher(lib, src.to(dev)), _float_reference(src), (t, h, w), kernel_case_shifts(*case),
              dev, f"warp_rigid_dma unaligned sum {(t, h, w)}", sum_offset=1, modes=("sum", "frames+sum"))


# ------------------------------------------------------------------ fp32: warp_rigid (register tile)


_REGISTER_PARAMS = [(c, "plain") if c[2] % 4 else (c, v) for c in KERNEL_CASES["warp_rigid"]
                    for v in (("plain",) if c[2] % 4 else ("frames pointer + 4 bytes", "out_frames + 4 bytes"))]


@pytest.mark.parametrize("case,variant", _REGISTER_PARAMS, ids=[f"{_case_id(c)}-{v}" for c, v in _REGISTER_PARAMS])
def test_warp_rigid_register_tile_matches_the_float64_resampler(lib, dev, case, variant):
    """The fallback kernel: w % 4 != 0 ((3, 130, 250), (2, 96, 1030)), and w % 4 == 0 with the frames -- or only
    out_frames -- one float off a 16-byte boundary, where dma_ok is false although the rows are whole quads."""
    t, h, w = case[:3]
    src = float_stack(t, h, w)
    sd = src.to(dev) if variant != "frames pointer + 4 bytes" else offset_copy(src.to(dev), 1)
    assert sd.data_ptr() % 16 == (4 if variant == "frames pointer + 4 bytes" else 0)
    launch = _float_launcher(lib, sd)
    shifts = kernel_case_shifts(*case)
    _run_case(lib, launch, _float_reference(src), (t, h, w), shifts, dev, f"warp_rigid {(t, h, w)} {variant}",
              frames_offset=1 if variant == "out_frames + 4 bytes" else 0)
    if variant != "out_frames + 4 bytes":
        _assert_phases_split(lib, launch, (t, h, w), shifts, dev, f"warp_rigid phases {variant}")


# ------------------------------------------------------------------ fp16: warp_rigid_dma_h


@pytest.mark.parametrize("case", KERNEL_CASES["warp_rigid_dma_h"], ids=_case_id)
def test_warp_rigid_dma_h_matches_the_float64_resampler(lib, dev, case):
    """fp16 frames, both window parities P (the x shifts' integer parts are of both parities, host-asserted):
    (3, 33, 520) partial tiles, (3, 64, 2048) the remap, (2, 1024, 4096), (3, 40, 1032) w % 8 == 0 but no multiple
    of 512.  The bound is the fp32 one on the up-cast values.  The first case also runs the phase split, the last
    one an unaligned sum."""
    t, h, w = case[:3]
    src = float_stack(t, h, w, torch.float16)
    launch = _float_launcher(lib, src.to(dev))
    shifts = kernel_case_shifts(*case)
    _run_case(lib, launch, _float_reference(src), (t, h, w), shifts, dev, f"warp_rigid_dma_h {(t, h, w)}")
    if case == KERNEL_CASES["warp_rigid_dma_h"][0]:
        _assert_phases_split(lib, launch, (t, h, w), shifts, dev, "warp_rigid_dma_h phases")
    if case == KERNEL_CASES["warp_rigid_dma_h"][-1]:
        _run_case(lib, launch, _float_reference(src), (t, h, w), shifts[:t], dev,
                  f"warp_rigid_dma_h unaligned sum {(t, h, w)}", sum_offset=1, modes=("sum", "frames+sum"))


# ------------------------------------------------------------------ raw u8 / i16: warp_rigid_raw


_RAW_PARAMS = [(case, dtype) for case in KERNEL_CASES["warp_rigid_raw"] for dtype in (torch.uint8, torch.int16)
               if not (dtype == torch.int16 and case[1] == 4096)]  # 4096^2: u8 only


@pytest.mark.parametrize("with_gain", [True, False], ids=["gain", "no gain"])
@pytest.mark.parametrize("case,dtype", _RAW_PARAMS, ids=[f"{_case_id(c)}-{str(d)[6:]}" for c, d in _RAW_PARAMS])
def test_warp_rigid_raw_matches_the_float64_resampler(lib, dev, case, dtype, with_gain):
    """u8 (sub-unit offsets m = 0..3) and i16 (m = 0, 1) frames with a gain of large dynamic range, and without
    one, against the float64 conditioning + resampler; mu and kind come from engine.RawMovie.  (6, 33, 516) also
    runs the phase split and an unaligned sum."""
    t, h, w = case[:3]
    raw, gain, rm = raw_setup(dev, t, h, w, dtype, with_gain, seed=500 + h)
    launch = _raw_launcher(lib, rm)
    reference = _raw_reference(raw, gain, rm.mu.cpu().numpy())
    shifts = kernel_case_shifts(*case)
    what = f"warp_rigid_raw {str(dtype)[6:]} {(t, h, w)} {'gain' if with_gain else 'no gain'}"
    _run_case(lib, launch, reference, (t, h, w), shifts, dev, what)
    if case == KERNEL_CASES["warp_rigid_raw"][0]:
        _assert_phases_split(lib, launch, (t, h, w), shifts, dev, what + " phases")
        _run_case(lib, launch, reference, (t, h, w), shifts[:t], dev, what + " unaligned sum", sum_offset=1,
                  modes=("sum", "frames+sum"))


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16], ids=["uint8", "int16"])
def test_warp_rigid_raw_gain_cache_recentring(lib, dev, dtype):
    """The integer parts of consecutive frames' shifts jump by +5, +9, -9, -20, +20 in y, then in x, then on both
    axes at once and return to the start (rigid_reference.RECENTRE_SHIFTS): the gain cache, centred with 8 spare
    rows and columns, is kept, re-centred and re-used.  Gain in [0.25, 4]; one full tile + edge tiles."""
    t, h, w = len(RECENTRE_SHIFTS), 72, 1028
    raw, gain, rm = raw_setup(dev, t, h, w, dtype, True, seed=640)
    _run_case(lib, _raw_launcher(lib, rm), _raw_reference(raw, gain, rm.mu.cpu().numpy()), (t, h, w),
              RECENTRE_SHIFTS, dev, f"warp_rigid_raw {str(dtype)[6:]} recentring")


def test_warp_rigid_raw_at_its_frame_limit(lib, dev):
    """t = 256 = RR_PAR_MAX frames on (256, 64, 512) u8: the last slot of the per-frame parameter table."""
    t, h, w = 256, 64, 512
    raw, gain, rm = raw_setup(dev, t, h, w, torch.uint8, True, seed=256)
    shifts = kernel_case_shifts(t, h, w, offset=3, n_pool=t - 4)
    assert len(shifts) == t
    _run_case(lib, _raw_launcher(lib, rm), _raw_reference(raw, gain, rm.mu.cpu().numpy()), (t, h, w), shifts, dev,
              "warp_rigid_raw uint8 t=256")


def test_raw_route_beyond_the_frame_limit_falls_back(mc, lib, dev):
    """t = 257: mc_warp_rigid_raw answers MC_ERR_UNSUPPORTED (before any launch) and motion_correct_sum_raw falls
    back to conditioning + the fp32 route.  Against the same reference with the same bound (fp32 term + conditioning
    term); the shifts are the lattice the route evaluates over fp32(ps), read back."""
    from torch_motion_correction_amd import engine
    from torch_motion_correction_amd._lib import ptr, stream_ptr

    t, h, w, ps = 257, 64, 512, 0.83
    raw, gain, rm = raw_setup(dev, t, h, w, torch.uint8, True, seed=257)
    px = torch.from_numpy(kernel_case_shifts(t, h, w, offset=5, n_pool=t - 4).copy())
    scratch = _scratch(lib, t, h, w, dev)
    total, _ = nan_buffer((h, w), dev)
    rc = lib.mc_warp_rigid_raw(ptr(rm.raw), rm.kind, ptr(rm.gain), ptr(rm.mu), t, h, w, ptr(px.to(dev)), ptr(scratch),
                               None, ptr(total), 0, stream_ptr(dev))
    assert rc == -2 and bool(torch.isnan(total).all())
    field = mc.image_shifts_to_deformation_field(px, ps).contiguous()
    s, fr = mc.motion_correct_sum_raw(raw.to(dev), gain.to(dev), field.to(dev), ps, return_frames=True)
    torch.cuda.synchronize()
    sh = engine.frame_lattices(field.to(dev), t, "catmull_rom")[:, :, 0, 0].cpu().numpy() / np.float32(ps)
    ref, bound = _raw_reference(raw, gain, rm.mu.cpu().numpy())(sh.astype(np.float32))
    rf = assert_frames(fr, ref, bound, "motion_correct_sum_raw t=257 frames")
    rs = assert_sum(s, ref.sum(0), _sum_bound(ref, bound), "motion_correct_sum_raw t=257 sum")
    print(f"RATIO motion_correct_sum_raw t=257 (fallback): frames {rf:.3f} sum {rs:.3f}")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16], ids=["uint8", "int16"])
def test_warp_rigid_raw_accumulate_sums_two_chunks(lib, dev, dtype):
    """mc_warp_rigid_raw_accumulate: two chunks of 3 frames of one (6, 64, 2048) movie into one zeroed buffer, with
    and without frames.  Reference = the sum of both chunks' references; bound = both chunks' sum bounds + one fp32
    add per pixel for the second chunk (the first is added to zero, exactly)."""
    t, h, w, n = 6, 64, 2048, 3
    raw, gain, rm = raw_setup(dev, t, h, w, dtype, True, seed=77)
    mu = rm.mu.cpu().numpy()
    shifts = kernel_case_shifts(t, h, w, offset=6, n_pool=2)
    want, bound = np.zeros((h, w)), np.zeros((h, w))
    refs = []
    for a in (0, n):
        ref, fb = _raw_reference(raw[a:a + n], gain, mu[a:a + n])(shifts[a:a + n])
        refs.append((ref, fb))
        want += ref.sum(0)
        bound += _sum_bound(ref, fb)
    bound += ULP * (np.abs(refs[0][0].sum(0)) + np.abs(refs[1][0].sum(0)) + bound)
    for with_frames in (False, True):
        total, total_all = nan_buffer((h, w), dev)
        total.zero_()
        for i, a in enumerate((0, n)):
            win = rm.window(a, n)
            frames, frames_all = nan_buffer((n, h, w), dev) if with_frames else (None, None)
            sd = torch.from_numpy(np.ascontiguousarray(shifts[a:a + n])).to(dev)
            _raw_launcher(lib, win, accumulate=True)(sd, _scratch(lib, n, h, w, dev), frames, total, 0)
            torch.cuda.synchronize()
            if with_frames:
                assert_guards(frames, frames_all, "accumulate frames")
                assert_frames(frames, refs[i][0], refs[i][1], f"accumulate {dtype} chunk {i} frames")
        assert_guards(total, total_all, "accumulate sum")
        r = assert_sum(total, want, bound, f"accumulate {dtype} frames={with_frames}")
        print(f"RATIO mc_warp_rigid_raw_accumulate {str(dtype)[6:]} frames={with_frames}: sum {r:.3f}")
