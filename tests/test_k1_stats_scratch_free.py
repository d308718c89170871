"""The variants of the wave-per-row K1 (xc_rows_fwd_wave<KEEP, STATS, ...>) keep no state in scratch memory, and
still compute what they computed.

Host: csrc/xc_rows_fwd_wave.hip compiled for gfx950 with the library's flags; every instantiation's scratch size and
VGPR count read from the code object's metadata notes (nothing is disassembled).  There are 16 instantiations, the
ones an entry point can launch: 8 with statistics, 8 without.  Every one has 0 bytes of scratch, at most 256 VGPRs
and at most 40 KiB of LDS (four workgroups per CU).

GPU: mc_xc_rows_forward_stats_t called directly at the smallest shape the wave engine takes -- rows of 4096 samples,
64 rows (two rounds of WF_ROWS_PER_WG = 32 rows: the running sums are carried from round to round), 2 frames -- on a
hand-built geometry and mask, so that each of the eight statistics variants runs: fp32 with all 16 chunks of a row,
fp16, fp32 with the 14 inner chunks clamped to the support box or to per-row chords, each with at most 256 kept
bins (KEEP = 1) and with more (KEEP = 2).  The statistics box is on the 256-sample chunk grid and leaves rows of the
support outside it.  Inputs N(0, 1) and N(1000, 30^2), the latter because the provisional mean exists for it.

Judged against float64, with the bounds of tests/test_xc_kernels_float64.py for the same entry point and no other:

  statistics  |mean - mean64| <= 2 u |mean64| + 1e-7 std64, |std - std64| <= 8 u std64 (1 + |mean64| / std64), for
              both frames jointly and for each frame on its own (a call with that frame as its only job, whose T1 must
              be the joint call's, bit for bit).
  T1          xc_reference.check_spectra (L2 per job, CAP per bin) with the terms of xc_reference.spectra_bounds that
              apply to the row pass alone: what is transformed is (x - m0) mask with rstd = 1, so the normalisation
              term is (5 + d) u with d = |mean - m0| / std, the mask product rounds once (u; the float64 side takes
              the same fp32 mask values, so the table's own error drops out), the row transform costs
              line_costs(g)['rows_fwd'].  No column pass, no filter.  A bin's error scales with its own row's norm;
              the rows of these masks have the same norm to 2 %, so the per-bin statement uses their rms.

The eight variants without statistics (fp32 with all 16 chunks or the 14 inner ones, u8 and i16, each with KEEP 1 and
2): five run on 4096-column rows with 64 or more support rows in other tests -- fp32 all-16 with KEEP 1 and 2 in
test_xc_kernels_float64.py::test_wave_per_row_k1 ((2, 512, 4096), bands 20 and 10), fp32 inner with KEEP 2 in
test_gpu_parity.py::test_wave_row_engine_matches_workgroup_engine (h = 4096), u8 and i16 with KEEP 2 in
test_xc_kernels_float64.py::test_raw_movies ((2, 512, 4096)).  The other three run here, at the shapes above: fp32
inner with KEEP 1 through mc_xc_rows_forward, u8 and i16 with KEEP 1 through mc_xc_rows_forward_raw (gain in
[0.8, 1.2], an offset per frame).  Same judgement: check_spectra with (5 + |mean| / std) u for the normalisation
with supplied statistics (the `norm` term of xc_reference.spectra_bounds; raw input: mean 0), u for the mask product,
line_costs(g)['rows_fwd'], and for raw input the conditioning's rounding (rigid_reference.conditioning_error in L2
over the masked job, as tests/test_xc_kernels_float64.py::test_raw_movies adds it).
"""

import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import xc_reference as xr
from rigid_reference import condition_float64, conditioning_error
from kernel_harness import assert_guards, calls, nan_buffer  # noqa: F401

U = xr.U
T, H, W = 2, 64, 4096
BOX_W = (1024, 3072)  # wl, wu: whole 256-sample chunks


# ------------------------------------------------------------------ host: the code object's metadata


def _readelf():
    from torch_motion_correction_amd import _build

    rocm = os.path.dirname(os.path.dirname(os.path.realpath(_build.HIPCC)))
    for cand in (os.path.join(rocm, "llvm", "bin", "llvm-readelf"), os.path.join(rocm, "lib", "llvm", "bin", "llvm-readelf"),
                 "/opt/rocm/llvm/bin/llvm-readelf"):
        if os.path.exists(cand):
            return cand
    return shutil.which("llvm-readelf")


def test_statistics_variants_use_no_scratch(tmp_path):
    from torch_motion_correction_amd import _build

    tool = _readelf()
    if not os.path.exists(_build.HIPCC) or tool is None:
        pytest.skip("hipcc or llvm-readelf is not installed")
    flags = next(extra for src, _, extra in _build.SOURCES if src == "xc_rows_fwd_wave.hip")
    co = str(tmp_path / "xc_rows_fwd_wave.co")
    subprocess.run([_build.HIPCC, *_build.FLAGS, *flags, f"-I{_build.INCLUDE}", f"-I{_build.CSRC}", "--cuda-device-only",
                    "--no-gpu-bundle-output", "-c", os.path.join(_build.CSRC, "xc_rows_fwd_wave.hip"), "-o", co], check=True)
    notes = subprocess.run([tool, "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels = {}
    for block in re.split(r"\n\s*- \.", notes):  # one list item of amdhsa.kernels per kernel
        name = re.search(r"\.name:\s+(_Z16xc_rows_fwd_waveILi(\d)ELb([01])E\S*)", block)
        if name:
            field = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", block).group(1))  # noqa: E731
            kernels[name.group(1)] = (name.group(3) == "1", field("private_segment_fixed_size"), field("vgpr_count"),
                                      field("group_segment_fixed_size"))
    stats = {k: v for k, v in kernels.items() if v[0]}
    assert len(kernels) == 16 and len(stats) == 8, sorted(kernels)
    for name, (st, scratch, vgpr, lds) in sorted(kernels.items()):
        print(f"{name[:52]} scratch {scratch} vgpr {vgpr} lds {lds}")
        assert vgpr <= 256 and lds <= 40960, f"{name}: {vgpr} VGPRs, {lds} bytes of LDS"
        assert scratch == 0, f"{name}: {scratch} bytes of scratch per lane"


# ------------------------------------------------------------------ GPU: the eight variants against float64

# route -> (x0, x1, chords, fp16): which loads the variant rule of xc_rows_fwd.hip picks
ROUTES = {"all16": (0, 4096, False, False), "half": (0, 4096, True, True), "inner_box": (300, 3800, False, False),
          "inner_chord": (300, 3800, True, False)}
NKX = {1: 200, 2: 410}  # KEEP = 1: at most 256 kept bins; 2: the benchmark's 410


def _geometry(nkx, x0, x1, y0=0, ny=H):
    from torch_motion_correction_amd import _lib

    return _lib.XcGeom(W=W, H=H, nkx=nkx, kyp=8, kyn=7, y0=y0, ny=ny, x0=x0, x1=x1, RG=8)


def _mask(x0, x1, chords):
    """fp32 (H, W): values in [0.5, 1] on the support, exact zeros outside it; with `chords` every row's support is
    its own, 4-aligned and not narrower than the statistics box."""
    g = torch.Generator().manual_seed(x0 + 7 * x1 + chords)
    m = torch.rand(H, W, generator=g) * 0.5 + 0.5
    cols = torch.arange(W)[None, :]
    lo = torch.full((H, 1), x0)
    hi = torch.full((H, 1), x1)
    if chords:
        y = torch.arange(H)[:, None]
        lo = (x0 + 3) // 4 * 4 + 8 * (y % 5)
        hi = x1 // 4 * 4 - 8 * (y % 7)
    assert int(lo.max()) <= BOX_W[0] and int(hi.min()) >= BOX_W[1]
    return m * ((cols >= lo) & (cols < hi))


def _stats64(x, box):
    hl, hu, wl, wu = box
    b = x[:, hl:hu, wl:wu].double()
    return float(b.mean()), float(b.std())


def _run(lib, dev, xd, off, njobs, g, mask, chord, box, tw):
    """provisional mean + mc_xc_rows_forward_stats_t as engine._global_spectra issues them
    -> (T1 (njobs, nkx, ny, 2) on the CPU, out3 = (mean, 1 / std, std), m0)."""
    from torch_motion_correction_amd import engine
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    hl, hu, wl, wu = box
    st = stream_ptr(dev)
    acc = torch.empty(128, dtype=torch.float64, device=dev)
    m0 = torch.empty(3, dtype=torch.float32, device=dev)
    fix = torch.empty(2, dtype=torch.float32, device=dev)
    out3 = torch.empty(3, dtype=torch.float32, device=dev)
    first = int(off[0]) + hl * W + wl
    check(lib.mc_xc_provisional_mean_t(C.c_void_p(xd.data_ptr() + xd.element_size() * first), engine.storage_of(xd),
                                       wu - wl, ptr(m0), st), "mc_xc_provisional_mean_t")
    T1, flat = nan_buffer((njobs, g.nkx, g.ny, 2), dev)
    offd = off.to(dev)
    check(lib.mc_xc_rows_forward_stats_t(ptr(xd), engine.storage_of(xd), ptr(offd), W, ptr(mask), ptr(m0), ptr(T1),
                                         ptr(tw), njobs, g, hl, hu, wl, wu, ptr(acc), ptr(fix), ptr(out3),
                                         ptr(chord) if chord is not None else None, st), "mc_xc_rows_forward_stats_t")
    torch.cuda.synchronize()
    assert_guards(T1, flat, "T1")
    return T1.cpu(), out3.cpu().numpy().astype(np.float64), float(m0[0])


def _assert_stats(out3, m64, s64, what):
    print(f"  {what}: mean {out3[0]:.7g} (float64 {m64:.7g}), std {out3[2]:.7g} (float64 {s64:.7g})")
    assert abs(out3[0] - m64) <= 2 * U * abs(m64) + 1e-7 * s64, f"{what}: mean {out3[0]} against {m64}"
    assert abs(out3[2] - s64) <= 8 * U * s64 * (1 + abs(m64) / s64), f"{what}: std {out3[2]} against {s64}"


def _check(dev, calls, keep, route, mean, std, y0=0, ny=H, box_rows=(8, 56)):
    from torch_motion_correction_amd import plan

    x0, x1, chords, half = ROUTES[route]
    g = _geometry(NKX[keep], x0, x1, y0, ny)
    x = xr.noise(T, H, W, mean=mean, std=std, seed=keep)
    if half:
        x = x.half()
    mask = _mask(x0, x1, chords)
    maskd = mask.to(dev)
    chord = plan.row_chords(maskd) if chords else None
    tw = plan.get_twiddles(W, dev)
    box = (*box_rows, *BOX_W)
    xd = x.to(dev)
    what = f"KEEP {keep} {route} N({mean:g}, {std:g}^2) rows {y0}+{ny}"
    calls.clear()
    T1, out3, m0 = _run(calls, dev, xd, torch.arange(T, dtype=torch.int64) * (H * W), T, g, maskd, chord, box, tw)
    calls.ran("mc_xc_rows_forward_stats_t")
    m64, s64 = _stats64(x, box)
    _assert_stats(out3, m64, s64, what + " both frames")
    d = abs(m64 - m0) / s64
    assert d < 0.5, f"the provisional mean is {d:.2f} std from the mean"
    rel = (5 + d) * U + U + xr.line_costs(g)["rows_fwd"]
    xn = (x.double().numpy() - m0) * mask.double().numpy()[None]
    ref = np.ascontiguousarray(np.fft.rfft(xn[:, y0:y0 + ny], axis=2)[:, :, :g.nkx].transpose(0, 2, 1))
    parts = {"S": ref, "filt": np.ones(ref.shape[1:]),
             "rms": np.array([np.linalg.norm(xn[f, y0:y0 + ny]) / math.sqrt(ny) for f in range(T)])}
    r = xr.check_spectra(T1, parts, {"rel": rel, "fix_l2": 0.0, "fix_bin": 0.0}, what)
    print(f"RATIO K1 statistics variant {what}: L2 {r[0]:.3f} bin {r[1]:.3f}")
    for f in range(T):  # each frame as the only job of a call: its own statistics, the same T1
        T1f, out3f, _ = _run(calls, dev, xd, torch.tensor([f * H * W], dtype=torch.int64), 1, g, maskd, chord, box, tw)
        # (the provisional mean is the first box row of THIS frame: T1 equal bit for bit only where it is the same)
        _assert_stats(out3f, *_stats64(x[f:f + 1], box), f"{what} frame {f}")
        if f == 0:
            assert torch.equal(T1f[0], T1[0]), f"{what}: frame 0 alone differs from frame 0 of the joint call"


@pytest.mark.gpu
@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (1000.0, 30.0)])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("keep", [1, 2])
def test_statistics_variants_against_float64(dev, calls, keep, route, mean, std):
    """64 rows = two rounds of 32 per workgroup; the box rows 8 .. 56 leave rows of both rounds outside it."""
    _check(dev, calls, keep, route, mean, std)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["inner_chord", "all16"])
def test_last_workgroup_with_fewer_rows(dev, calls, route):
    """40 support rows from row 8: the route admits whole rounds of 8 rows, so the second workgroup has one round of 8
    rows instead of four -- every wave transforms one pair of rows there, and no sum of a round that did not run
    enters the statistics."""
    _check(dev, calls, 2, route, 1000.0, 30.0, y0=8, ny=40, box_rows=(16, 44))


# ------------------------------------------------------------------ GPU: the variants without statistics


def _check_plain(dev, calls, kind, y0=0, ny=H):
    """KEEP = 1 without statistics.  kind 'f32': the 14 inner chunks through mc_xc_rows_forward; 'u8' / 'i16': all 16
    chunks through mc_xc_rows_forward_raw."""
    from torch_motion_correction_amd import plan
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    raw = kind != "f32"
    x0, x1 = (0, 4096) if raw else (300, 3800)
    g = _geometry(NKX[1], x0, x1, y0, ny)
    mask = _mask(x0, x1, False)
    maskd = mask.to(dev)
    tw = plan.get_twiddles(W, dev)
    off = (torch.arange(T, dtype=torch.int64) * (H * W)).to(dev)
    st = stream_ptr(dev)
    T1, flat = nan_buffer((T, g.nkx, g.ny, 2), dev)
    what = f"KEEP 1 {kind} without statistics rows {y0}+{ny}"
    m64 = mask.double().numpy()[None]
    norm = lambda a: np.array([np.linalg.norm(a[f, y0:y0 + ny]) for f in range(T)])  # noqa: E731
    calls.clear()
    if raw:
        gen = torch.Generator().manual_seed(11 + (kind == "u8"))
        if kind == "u8":
            x = torch.clamp(torch.round(torch.randn(T, H, W, generator=gen) * 6 + 40), 0, 255).to(torch.uint8)
        else:
            x = torch.round(torch.randn(T, H, W, generator=gen) * 30 + 1000).to(torch.int16)
        gain = (0.8 + 0.4 * torch.rand(H, W, generator=gen)).float()
        v = x.double() * gain.double()
        sub = v.mean(dim=(1, 2)).float()  # an offset per frame
        stats = torch.tensor([0.0, 1.0 / float(v.std())], dtype=torch.float32)
        xd, gaind, subd, statsd = x.to(dev), gain.to(dev), sub.to(dev), stats.to(dev)
        check(calls.mc_xc_rows_forward_raw(ptr(xd), 0 if kind == "u8" else 1, ptr(gaind), ptr(off), W, ptr(maskd),  # MC_STORE_U8 / _I16
                                           ptr(subd), ptr(statsd), ptr(T1), ptr(tw), T, g, None, st),
              "mc_xc_rows_forward_raw")
        torch.cuda.synchronize()
        calls.ran("mc_xc_rows_forward_raw")
        c = condition_float64(x.numpy(), gain.numpy(), sub.numpy())
        xn = c * float(stats[1]) * m64
        cond = norm(conditioning_error(x.numpy(), gain.numpy(), sub.numpy()) * m64) / norm(c * m64)
        d = 0.0
    else:
        x = xr.noise(T, H, W, mean=5.0, std=2.0, seed=3)
        mean, std = float(x.double().mean()), float(x.double().std())
        stats = torch.tensor([mean, 1.0 / std], dtype=torch.float32)
        xd, statsd = x.to(dev), stats.to(dev)
        check(calls.mc_xc_rows_forward(ptr(xd), ptr(off), W, None, ptr(maskd), ptr(statsd), ptr(T1), ptr(tw), T, g, st),
              "mc_xc_rows_forward")
        torch.cuda.synchronize()
        calls.ran("mc_xc_rows_forward")
        xn = (x.double().numpy() - mean) / std * m64
        cond = np.zeros(T)
        d = abs(mean) / std
    assert_guards(T1, flat, "T1")
    ref = np.ascontiguousarray(np.fft.rfft(xn[:, y0:y0 + ny], axis=2)[:, :, :g.nkx].transpose(0, 2, 1))
    parts = {"S": ref, "filt": np.ones(ref.shape[1:]), "rms": norm(xn) / math.sqrt(ny)}
    rel = (5 + d) * U + U + xr.line_costs(g)["rows_fwd"]
    bounds = [{"rel": rel + float(cond[f]), "fix_l2": 0.0, "fix_bin": 0.0} for f in range(T)]
    r = xr.check_spectra(T1.cpu(), parts, bounds, what)
    print(f"RATIO K1 variant {what}: L2 {r[0]:.3f} bin {r[1]:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["f32", "u8", "i16"])
def test_variants_without_statistics_against_float64(dev, calls, kind):
    """The three instantiations without statistics that no other test launches on 4096-column rows (module
    docstring), on 64 rows = two workgroups of four store rounds."""
    _check_plain(dev, calls, kind)


@pytest.mark.gpu
def test_last_workgroup_with_fewer_rows_without_statistics(dev, calls):
    """40 support rows from row 8, u8 samples: the second workgroup runs one round of 8 rows instead of four."""
    _check_plain(dev, calls, "u8", y0=8, ny=40)
