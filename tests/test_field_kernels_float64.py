"""Every deformation-field warp kernel (csrc/warp_field.hip: warp_field3 fp32 / fp16 / raw u8 / raw i16 / ACCUM,
warp_field_plan, warp_field_slow; csrc/warp_field_fallback.hip: warp_main, warp_field2; csrc/field_tables.hip:
warp_axis_tables, warp_etab, warp_pixel_shifts, warp_pixel_shifts_at) against the float64
reference of tests/field_reference.py, through the C ABI with hand-made (t, 2, GH, GW) lattices: no spline, no
estimator, no knife-edge mask and no excluded pixel.

Every launch of a case runs the three output combinations -- frames, sum, frames + sum -- into NaN-filled buffers
with NaN guard words, scratch sized by mc_warp_scratch_bytes.  The frames of a case cycle through the lattice
families of field_reference.FAMILIES (zero, integer and fractional constants, smooth lattices of every margin class
mg = 2 .. 6, a rough lattice that is irregular on the tiles around one node only, a constant shift larger than a
tile, a shift >= n, a shift that leaves one row and one column); every group of frames is launched at ps = 1.0
(the UNIT_PS instantiations of the tile kernels and of warp_field_slow) and at 0.83 or 1.3, so every family meets
both.  Which route, margin classes, remap and irregular tile-frames each case reaches, at ps = 1.0 and at ps != 1.0
separately, is asserted from the dispatch rules on the host (tests/test_field_reference_host.py).

Bounds (derived in tests/field_reference.py and tests/rigid_reference.py, none fitted to a kernel's output):

  frames  a pixel lies within 32 * 2^-24 * mag + wterm [+ the resampled conditioning error for raw movies] of one of
          its candidates -- the float64 samples at the extreme fp32 coordinates of its shift interval (one candidate
          for almost every pixel) -- is exactly 0 where the coordinate is outside for the whole interval, and may be
          exactly 0 or such a value where the interval straddles the frame border, nothing else.  fp16: the bound on
          the up-cast values (the widening is exact).
  sum     the frames' intervals added, plus t roundings of the partial sums; tile-frames left to warp_field_slow
          are added to the stored sum with one more fp32 add per pixel; mc_warp_frames_raw_accumulate adds one
          more per chunk and pixel.

Measured worst |got - candidate| / bound over all cases of a route, from one run on an MI355X: frames (all pixels),
frames without the pixels that have a midpoint candidate, sum.  Recorded, not asserted:

  warp_main (also the unaligned stack)                      0.457   0.126   0.635
  warp_field2 + warp_field_slow                              0.701   0.103   0.809
  warp_field3 fp32 + warp_field_slow                         0.842   0.129   0.932   ((130, 33, 260): 0.651 0.120 0.065)
  warp_field3<HALF> + warp_field_slow<HALF>                  0.843   0.098   0.899
  warp_field3<RAW> u8 + warp_field_slow<RAW>                 0.961   0.196   0.966   ((130, 33, 272): 0.879 0.120 0.426)
  warp_field3<RAW> i16 + warp_field_slow<RAW>                0.951   0.184   0.966
  mc_warp_frames_raw_accumulate (u8, i16)                    -       -       0.821, 0.896
  mc_pixel_shifts, mc_pixel_shifts_at (ratio to es)          0.736, 0.577

  The sum column leaves out the pixels that are on the border in some frame (a kernel that writes the allowed 0
  there sits at the end of its interval by design; they are asserted like all others).  The large ratios of the first
  column all belong to midpoint candidates -- the border row / column of the integer-shift frames, |c| < 1e-6 --
  where the kernel's coordinate may be anywhere in [u_lo, u_hi] and the bound's leading term r D is the first-order
  effect of exactly that; everywhere else the headroom is that of the rigid kernels.

Arithmetic-only mutations of warp_field.hip (as one file, before it was split by job) / warp_common.h, each run once (new tests of this file that fail / the
older 1e-4 tests of test_gpu_parity.py and test_raw_local_motion.py):

  c[3] of cubic_coeffs_factored * (1 + 1e-5)                 0 of 34 / none.  |c3| <= 0.11, so the weight moves by
        <= 1.1e-6 = 18 * 2^-24, inside cubic_weight_error's 12 .. 27 * 2^-24 for a far tap: that term is derived for
        the Horner forms, whose far taps cancel; the factored form does not cancel and would allow a far-tap term of a
        few ulps of the weight itself.  The bound is the rigid one by specification; tightening wterm for the
        kernels that use the factored weights is what would catch this mutation.
  sx * (1 + 2e-6) in the rim body of warp_field3 only        26 of 34 (every warp_field3 test) / none
  RAW widening pass rounding raw * gain - m through fp16     17 of 34 (every raw test) / 8 (test_field_warp_from_raw_bytes)
"""

import ctypes as C

import numpy as np
import pytest
import torch

from field_reference import (ACCUM_CASES, ACCUM_RUNS, ACCUM_SPACINGS, CASE_STORAGE, FAMILIES, FIELD_CASES, ULP,
                             accumulate_lattices, case_launches, case_lattices, field_reference, shift_at,
                             shift_interval, sum_reference, tile_plan)
from kernel_harness import (assert_guards, assert_sum, float_stack, lib, nan_buffer, offset_copy,  # noqa: F401
                            raw_setup)
from rigid_reference import condition_float64, conditioning_error

pytestmark = pytest.mark.gpu

MODES = ("frames", "sum", "frames+sum")
MC_ERR_ARG, MC_ERR_UNSUPPORTED = -1, -2


# ------------------------------------------------------------------ buffers and launches


def _scratch(lib, t, h, w, GH, GW, dev):
    from torch_motion_correction_amd._lib import check

    nbytes = C.c_int64(0)
    check(lib.mc_warp_scratch_bytes(t, h, w, GH, GW, C.byref(nbytes)), "mc_warp_scratch_bytes")
    s = torch.zeros((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)
    assert s.data_ptr() % 16 == 0
    return s


def _float_launcher(lib, src):
    """launch(lattice, ps, scratch, frames, total) -> return code of mc_warp_frames_t over the fp32 / fp16 stack."""
    from torch_motion_correction_amd import engine
    from torch_motion_correction_amd._lib import ptr, stream_ptr

    t, h, w = src.shape
    storage = engine.storage_of(src)

    def launch(lat, ps, scratch, frames, total):
        _, _, GH, GW = lat.shape
        return lib.mc_warp_frames_t(ptr(src), storage, t, h, w, ptr(lat), GH, GW, float(ps), ptr(scratch), ptr(frames),
                                    ptr(total), stream_ptr(src.device))

    return launch


def _raw_launcher(lib, rm, accumulate=False):
    from torch_motion_correction_amd._lib import ptr, stream_ptr

    t, h, w = rm.shape
    entry = lib.mc_warp_frames_raw_accumulate if accumulate else lib.mc_warp_frames_raw

    def launch(lat, ps, scratch, frames, total):
        _, _, GH, GW = lat.shape
        return entry(ptr(rm.raw), rm.kind, ptr(rm.gain), ptr(rm.mu), t, h, w, ptr(lat), GH, GW, float(ps), ptr(scratch),
                     ptr(frames), ptr(total), stream_ptr(rm.raw.device))

    return launch


# ------------------------------------------------------------------ inputs and references


def _float_reference(src):
    values = src.float().numpy().astype(np.float64)
    return lambda lat, ps: field_reference(values, lat, ps)


def _raw_reference(raw, gain, mu):
    """The float64 conditioning with the kernel's own fp32 frame means (engine.RawMovie.mu read back) and the
    conditioning's rounding as a per-sample error map."""
    raw_np = raw.numpy()
    gain_np = None if gain is None else gain.numpy()
    mu_np = np.asarray(mu, dtype=np.float32)
    v = condition_float64(raw_np, gain_np, mu_np)
    assert not (v == 0).any(), "a conditioned sample is exactly zero: pick another gain / movie"
    err = conditioning_error(raw_np, gain_np, mu_np)
    return lambda lat, ps, a=0, n=None: field_reference(v[a:a + (n or len(v))], lat, ps, err=err[a:a + (n or len(v))])


def _run_case(lib, launch, reference, case, dev, what, slow=True):
    """Every launch of the case x every output combination; the reference is computed once per launch.  `slow`:
    the route has a warp_field_slow pass (one more add per pixel of the sum)."""
    from torch_motion_correction_amd._lib import check

    t, h, w, GH, GW = case
    scratch = _scratch(lib, t, h, w, GH, GW, dev)
    worst_f = worst_s = worst_p = 0.0
    for no, ps in case_launches(case):
        lat = case_lattices(case, ps, no)
        ld = torch.from_numpy(lat).to(dev)
        ref = reference(lat, ps)
        want, sum_bound = sum_reference(ref, 1 if slow else 0)
        for mode in MODES:
            tag = f"{what} launch {no} ps {ps} [{mode}]"
            frames, frames_all = nan_buffer((t, h, w), dev) if "frames" in mode else (None, None)
            total, total_all = nan_buffer((h, w), dev) if "sum" in mode else (None, None)
            check(launch(ld, ps, scratch, frames, total), tag)
            torch.cuda.synchronize()
            if frames is not None:
                assert_guards(frames, frames_all, tag)
                worst_f = max(worst_f, ref.check(frames.cpu().numpy(), tag))
                worst_p = max(worst_p, ref.worst_plain)
            if total is not None:
                assert_guards(total, total_all, tag)
                worst_s = max(worst_s, assert_sum(total, want, sum_bound, tag, ref.border.any(0)))
    print(f"RATIO {what}: frames {worst_f:.3f} (without midpoint candidates {worst_p:.3f}) sum {worst_s:.3f}")


def _case_id(case):
    return "x".join(str(v) for v in case)


# ------------------------------------------------------------------ fp32 routes


@pytest.mark.parametrize("case", FIELD_CASES["warp_main"], ids=_case_id)
def test_warp_main_matches_the_float64_reference(lib, dev, case):
    """w % 4 != 0: the untiled kernel (its 5 x 8 register window and its clipped-tap branch)."""
    src = float_stack(*case[:3])
    _run_case(lib, _float_launcher(lib, src.to(dev)), _float_reference(src), case, dev, f"warp_main {case}", slow=False)


@pytest.mark.parametrize("case", FIELD_CASES["warp_main_unaligned"], ids=_case_id)
def test_warp_main_takes_an_unaligned_stack(lib, dev, case):
    """w % 4 == 0 but `frames` one float past a 16-byte boundary: routed to warp_main."""
    src = float_stack(*case[:3])
    sd = offset_copy(src.to(dev), 1)
    assert sd.data_ptr() % 16 == 4
    _run_case(lib, _float_launcher(lib, sd), _float_reference(src), case, dev, f"warp_main unaligned {case}", slow=False)


@pytest.mark.parametrize("case", FIELD_CASES["warp_field2"], ids=_case_id)
def test_warp_field2_matches_the_float64_reference(lib, dev, case):
    """A lattice denser than 1.5 cells per 32 rows: warp_field2 + warp_field_slow."""
    src = float_stack(*case[:3])
    _run_case(lib, _float_launcher(lib, src.to(dev)), _float_reference(src), case, dev, f"warp_field2 {case}")


@pytest.mark.parametrize("case", FIELD_CASES["warp_field3"], ids=_case_id)
def test_warp_field3_matches_the_float64_reference(lib, dev, case):
    """The production kernel on fp32 frames: partial last tiles, exactly one tile, 16 tiles (remap) and 18 (none),
    interior and rim tile-frames, the clipped-column patch, 130 frames (the second plan block)."""
    src = float_stack(*case[:3])
    _run_case(lib, _float_launcher(lib, src.to(dev)), _float_reference(src), case, dev, f"warp_field3 {case}")


# ------------------------------------------------------------------ fp16


@pytest.mark.parametrize("case", FIELD_CASES["warp_field3_half"], ids=_case_id)
def test_warp_field3_half_matches_the_float64_reference(lib, dev, case):
    """fp16 frames (exact fp16 values, none zero) through warp_field3<HALF> and warp_field_slow<HALF>; the
    reference and the bound are taken on the up-cast."""
    src = float_stack(*case[:3], dtype=torch.float16)
    _run_case(lib, _float_launcher(lib, src.to(dev)), _float_reference(src), case, dev, f"warp_field3<HALF> {case}")


# ------------------------------------------------------------------ raw u8 / i16

# the 130-frame movie runs with the gain only
_RAW_PARAMS = [(c, d, g) for d, key in ((torch.uint8, "warp_field3_u8"), (torch.int16, "warp_field3_i16"))
               for c in FIELD_CASES[key] for g in (True, False) if g or c[0] < 100]


@pytest.mark.parametrize("case,dtype,with_gain", _RAW_PARAMS,
                         ids=[f"{_case_id(c)}-{str(d)[6:]}-{'gain' if g else 'no gain'}" for c, d, g in _RAW_PARAMS])
def test_warp_field3_raw_matches_the_float64_reference(lib, dev, case, dtype, with_gain):
    """Raw frames through warp_field3<RAW> + warp_field_slow<RAW> with a gain of large dynamic range and with the
    all-ones gain, against the float64 conditioning (mu read back from engine.RawMovie) + resampler."""
    t, h, w = case[:3]
    raw, gain, rm = raw_setup(dev, t, h, w, dtype, with_gain, seed=700 + h + w)
    _run_case(lib, _raw_launcher(lib, rm), _raw_reference(raw, gain, rm.mu.cpu().numpy()), case, dev,
              f"warp_field3<RAW> {str(dtype)[6:]} {case} {'gain' if with_gain else 'no gain'}")


@pytest.mark.parametrize("ps", ACCUM_SPACINGS)
@pytest.mark.parametrize("dtype,kind", [(torch.uint8, "u8"), (torch.int16, "i16")], ids=["uint8", "int16"])
def test_warp_frames_raw_accumulate_sums_chunks(lib, dev, dtype, kind, ps):
    """A 6-frame movie warped in two and in three chunks: the first by mc_warp_frames_raw (it stores the sum), the
    others by mc_warp_frames_raw_accumulate onto it, against the float64 sum of all frames; one more fp32 add per
    chunk and pixel; at ps = 1.0 (UNIT_PS) and 0.83.  The two-chunk run has no irregular tile-frame (asserted from
    the plan rule): it runs twice and the two sums are bit-equal.  The three-chunk run has irregular tile-frames
    (warp_field_slow adds to the accumulated sum).  Lattices: field_reference.ACCUM_RUNS (their on-border caps are
    asserted on the host)."""
    from torch_motion_correction_amd._lib import check

    case = ACCUM_CASES[kind]
    t, h, w, GH, GW = case
    raw, gain, rm = raw_setup(dev, t, h, w, dtype, True, seed=77)
    reference = _raw_reference(raw, gain, rm.mu.cpu().numpy())
    for run, (families, n) in enumerate(ACCUM_RUNS):
        lat = accumulate_lattices(case, families, ps)
        irregular = tile_plan(lat, h, w, ps)[0] == 0
        assert irregular.any() == (run == 1)
        want, bound, refs, edge = np.zeros((h, w)), np.zeros((h, w)), [], np.zeros((h, w), dtype=bool)
        for a in range(0, t, n):
            ref = reference(lat[a:a + n], ps, a, n)
            refs.append(ref)
            edge |= ref.border.any(0)
            cw, cb = sum_reference(ref, 1)
            want += cw
            bound += cb
        absum = sum(np.abs(r.center).sum(0) + r.radius.sum(0) for r in refs)
        bound = bound + len(refs) * ULP * (absum + bound)  # one add of partial sums <= absum + bound per chunk
        sums = []
        for rep in range(2 if run == 0 else 1):
            for with_frames in (False, True):
                total, total_all = nan_buffer((h, w), dev)
                for i, a in enumerate(range(0, t, n)):
                    win = rm.window(a, n)
                    frames, frames_all = nan_buffer((n, h, w), dev) if with_frames else (None, None)
                    ld = torch.from_numpy(lat[a:a + n]).to(dev)
                    check(_raw_launcher(lib, win, accumulate=i > 0)(ld, ps, _scratch(lib, n, h, w, GH, GW, dev), frames,
                                                                    total), "mc_warp_frames_raw(_accumulate)")
                    torch.cuda.synchronize()
                    if with_frames:
                        assert_guards(frames, frames_all, "accumulate frames")
                        refs[i].check(frames.cpu().numpy(), f"accumulate {dtype} chunk {i} frames")
                assert_guards(total, total_all, "accumulate sum")
                r = assert_sum(total, want, bound, f"accumulate {dtype} chunks of {n} ps {ps} frames={with_frames}", edge)
                print(f"RATIO mc_warp_frames_raw_accumulate {str(dtype)[6:]} chunks of {n} ps {ps} frames={with_frames}: sum {r:.3f}")
                sums.append(total.clone())
        for s in sums[1:]:
            if run == 0:
                assert torch.equal(s, sums[0]), "a sum without irregular tile-frames is not reproducible to the bit"


# ------------------------------------------------------------------ argument contract


def test_argument_contract_before_any_launch(lib, dev):
    """What the entry points refuse, and that a refusal writes nothing."""
    from torch_motion_correction_amd import engine
    from torch_motion_correction_amd._lib import ptr, stream_ptr

    def outputs(t, h, w):
        return nan_buffer((t, h, w), dev)[0], nan_buffer((h, w), dev)[0]

    def untouched(frames, total):
        torch.cuda.synchronize()
        return bool(torch.isnan(frames).all()) and bool(torch.isnan(total).all())

    ps = 0.83
    # fp16: rows of whole 8-sample units, the sparse lattice, a 16-byte aligned stack
    for (t, h, w, GH, GW), offset in (((3, 33, 260, 2, 3), 0), ((3, 33, 264, 8, 5), 0), ((3, 33, 264, 2, 3), 1)):
        src = float_stack(t, h, w, torch.float16).to(dev)
        src = offset_copy(src, offset) if offset else src
        assert src.data_ptr() % 16 == 2 * offset
        lat = torch.from_numpy(case_lattices((t, h, w, GH, GW), ps, 0)).to(dev)
        frames, total = outputs(t, h, w)
        rc = _float_launcher(lib, src)(lat, ps, _scratch(lib, t, h, w, GH, GW, dev), frames, total)
        assert rc == MC_ERR_UNSUPPORTED and untouched(frames, total), (t, h, w, GH, GW, offset, rc)
    # raw: rows of whole 16-byte units
    for dtype, w in ((torch.uint8, 264), (torch.int16, 260)):
        t, h, GH, GW = 3, 33, 2, 3
        _, _, rm = raw_setup(dev, t, h, w, dtype, True, seed=3)
        lat = torch.from_numpy(case_lattices((t, h, w, GH, GW), ps, 0)).to(dev)
        for acc in (False, True):
            frames, total = outputs(t, h, w)
            rc = _raw_launcher(lib, rm, acc)(lat, ps, _scratch(lib, t, h, w, GH, GW, dev), frames, total)
            assert rc == MC_ERR_UNSUPPORTED and untouched(frames, total), (dtype, w, acc, rc)
    # accumulate needs a sum; scratch must be 16-byte aligned
    t, h, w, GH, GW = 3, 33, 272, 2, 3
    _, _, rm = raw_setup(dev, t, h, w, torch.uint8, True, seed=4)
    lat = torch.from_numpy(case_lattices((t, h, w, GH, GW), ps, 0)).to(dev)
    frames, total = outputs(t, h, w)
    scratch = _scratch(lib, t, h, w, GH, GW, dev)
    assert _raw_launcher(lib, rm, True)(lat, ps, scratch, frames, None) == MC_ERR_ARG and untouched(frames, total)
    big = torch.zeros(scratch.numel() + 4, dtype=torch.float32, device=dev)
    off = big[1:1 + scratch.numel()]
    assert off.data_ptr() % 16 == 4
    assert _raw_launcher(lib, rm, False)(lat, ps, off, frames, total) == MC_ERR_ARG and untouched(frames, total)
    assert _raw_launcher(lib, rm, True)(lat, ps, off, frames, total) == MC_ERR_ARG and untouched(frames, total)
    src = float_stack(t, h, w).to(dev)
    assert _float_launcher(lib, src)(lat, ps, off, frames, total) == MC_ERR_ARG and untouched(frames, total)
    out = torch.full((h, w, 2), float("nan"), device=dev)
    assert lib.mc_pixel_shifts(ptr(lat[0]), GH, GW, h, w, ps, ptr(off), ptr(out), stream_ptr(dev)) == MC_ERR_ARG
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert engine.storage_of(src) == 3


# ------------------------------------------------------------------ pixel shifts


@pytest.mark.parametrize("case", [FIELD_CASES["warp_field3"][2], FIELD_CASES["warp_field2"][1]], ids=_case_id)
def test_pixel_shifts_lie_in_the_reference_interval(lib, dev, case):
    """mc_pixel_shifts (E table + the y dot product) within es of the reference's shift; mc_pixel_shifts_at (the
    direct 16-tap form, field_reference.shift_at) at the pixel centres and at fractional coordinates, some outside
    the frame, within its own bound."""
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    t, h, w, GH, GW = case
    worst = worst_at = 0.0
    for no, ps in case_launches(case):
        lat = case_lattices(case, ps, no)
        s, es = shift_interval(lat, h, w, ps)
        rng = np.random.default_rng(no)
        yy, xx = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
        grid = np.stack([yy, xx], -1).reshape(-1, 2)
        scattered = (rng.uniform(-0.1, 1.1, size=(4096, 2)) * [h - 1, w - 1]).astype(np.float32)
        coords = np.concatenate([grid, scattered])
        cd = torch.from_numpy(coords).to(dev)
        for f in range(t):
            ld = torch.from_numpy(lat[f]).to(dev)
            out = torch.full((h, w, 2), float("nan"), device=dev)
            check(lib.mc_pixel_shifts(ptr(ld), GH, GW, h, w, float(ps), ptr(_scratch(lib, 1, h, w, GH, GW, dev)), ptr(out),
                                      stream_ptr(dev)), "mc_pixel_shifts")
            at = torch.full((len(coords), 2), float("nan"), device=dev)
            check(lib.mc_pixel_shifts_at(ptr(ld), GH, GW, h, w, float(ps), ptr(cd), len(coords), ptr(at),
                                         stream_ptr(dev)), "mc_pixel_shifts_at")
            torch.cuda.synchronize()
            d = np.abs(out.cpu().double().numpy() - s[f].transpose(1, 2, 0))
            b = es[f].transpose(1, 2, 0)
            assert bool((d <= b).all()), (no, ps, f, float(d.max()), np.argwhere(~(d <= b))[:4].tolist())
            sa, ea = shift_at(lat[f], h, w, ps, coords)
            da = np.abs(at.cpu().double().numpy() - sa)
            assert bool((da <= ea).all()), (no, ps, f, float(da.max()), np.argwhere(~(da <= ea))[:4].tolist())
            with np.errstate(divide="ignore", invalid="ignore"):
                worst = max(worst, float(np.nan_to_num(d / b, nan=0.0, posinf=0.0).max()))
                worst_at = max(worst_at, float(np.nan_to_num(da / ea, nan=0.0, posinf=0.0).max()))
    print(f"RATIO pixel shifts {case}: mc_pixel_shifts {worst:.3f} mc_pixel_shifts_at {worst_at:.3f}")


assert len(FAMILIES) == 12 and set(CASE_STORAGE) == set(FIELD_CASES)
