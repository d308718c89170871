"""CPU tests of the product's host logic (no GPU, no compute calls into libmcorr):
lattice + memo replay pinned by the reference's goldens, pruning geometry proven
conservative against the oracle's filters/mask, spline tap tables against the
oracle's spline, C-ABI symbol export, and world_size-2 gloo sharding."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle
from kernel_harness import declared_entry_points, run_host_program
from oracle import thirdparty_semantics as tp
from torch_motion_correction_amd import _lib, lattice, multi_gpu, plan, spline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ lattice / memo replay


def test_patch_centres_match_reference(golden):
    g = golden("patch_grid_reference.npz")
    for key in g.files:
        if key.startswith("centers_"):
            _, dim, p = key.split("_")
            assert np.array_equal(lattice.patch_centers_1d(int(dim), int(p), int(p) // 2), g[key]), key


def test_baseline_config_lattices():
    """SURVEY.md section 8 header: p=1024 -> C2 6x6, C3 6x10, C5 14x21."""
    assert [len(a) for a in lattice.patch_grid_centers(40, 4096, 4096, 1024)] == [6, 6]
    assert [len(a) for a in lattice.patch_grid_centers(40, 4092, 5760, 1024)] == [6, 10]
    assert [len(a) for a in lattice.patch_grid_centers(60, 8184, 11520, 1024)] == [14, 21]
    cy, _ = lattice.patch_grid_centers(40, 4096, 4096, 1024)
    assert cy.tolist() == [512, 1126, 1740, 2355, 2969, 3583]


@pytest.mark.parametrize("t", [5, 8, 40, 51, 60])
@pytest.mark.parametrize("strategy", ["middle_frame", "mean_except_current"])
def test_mask_schedule_matches_reference(golden, t, strategy):
    g = golden("patch_grid_reference.npz")
    ref_expo, cur_expo, processed = lattice.mask_schedule(t, strategy, t // 2)
    assert np.array_equal(ref_expo, g[f"exp_{strategy}_{t}"])
    assert np.array_equal(cur_expo, g[f"cur_{strategy}_{t}"])
    expect = [f for f in range(t) if not (strategy == "middle_frame" and f == t // 2)]
    assert processed == expect


def test_mask_schedule_unknown_strategy():
    with pytest.raises(ValueError, match="Unknown reference_strategy"):
        lattice.mask_schedule(5, "nope", 2)


def test_centers_tensor_layout():
    cy, cx = lattice.patch_grid_centers(3, 64, 96, 32)
    c = lattice.centers_tensor(3, cy, cx)
    assert c.shape == (3, len(cy), len(cx), 3) and c.dtype == torch.int64
    assert c[2, 1, 0].tolist() == [2, int(cy[1]), int(cx[0])]


# ------------------------------------------------------------------ pruning geometry


@pytest.mark.parametrize("n,ps,fr", [(64, 1.0, (300, 10)), (256, 1.0, (300, 10)), (512, 0.83, (300, 10)),
                                     (128, 1.5, (200, 20)), (64, 6.0, (300, 10))])
def test_geometry_is_a_superset_of_the_filter_support(n, ps, fr):
    low, high = plan.band_limits(fr, ps)
    g = plan.xc_geometry(n, n, high, n / 4, n / 8)
    filt = oracle.prepare_bandpass_filter(fr, (n, n), ps) * tp.b_envelope(500, (n, n), ps)
    rows = list(range(g.kyp)) + list(range(n - g.kyn, n))
    outside = filt.clone()
    outside[rows, : g.nkx] = 0
    assert float(outside.abs().max()) == 0.0, "a non-zero filter bin would be pruned away"
    assert g.kyp + g.kyn <= n and 1 <= g.nkx <= n // 2 + 1
    mask = tp.circle(n / 4, (n, n), smoothing_radius=n / 8)
    outside = mask.clone()
    outside[g.y0 : g.y0 + g.ny, g.x0 : g.x1] = 0
    assert float(outside.abs().max()) == 0.0, "a non-zero mask pixel would never be read"
    assert g.ny % g.RG == 0 and n % g.RG == 0 and g.x0 % 2 == 0 and g.x1 % 2 == 0


def test_headline_geometry_prunes():
    """40x4096^2 at 1 A/px, (300,10) A: ~10 % of the columns, ~20 % of the rows kept."""
    low, high = plan.band_limits((300, 10), 1.0)
    g = plan.xc_geometry(4096, 4096, high, 1024, 512)
    assert (g.nkx, g.kyp, g.kyn) == (410, 410, 409)
    assert g.ny <= 3104 and g.x1 - g.x0 <= 3104


def test_full_geometry_keeps_everything():
    g = plan.full_geometry(64, 128)
    assert (g.nkx, g.kyp, g.kyn, g.y0, g.ny, g.x0, g.x1) == (65, 64, 0, 0, 64, 0, 128)


def test_unsupported_sizes_fail_loudly():
    with pytest.raises(NotImplementedError, match="even widths"):
        plan.xc_geometry(4092, 8193, 0.1, 1000, 500)  # odd widths: one sample per line point, at most 8191
    assert plan.xc_geometry(959, 927, 0.1, 927 / 4, 927 / 8).nkx == 93  # the reference's example movie size
    with pytest.raises(NotImplementedError, match="even widths"):
        plan.xc_geometry(8200, 11520, 0.1, 2000, 1000)  # beyond the 8192-row limit
    with pytest.raises(NotImplementedError, match="even widths"):
        plan.xc_geometry(4096, 16400, 0.1, 1000, 500)  # beyond the 16384-column limit
    with pytest.raises(NotImplementedError, match="M="):
        plan.line_plan(8200, -1, "cpu")
    with pytest.raises(NotImplementedError, match="160 KB"):
        plan.full_geometry(8184, 11520)  # the full spectrum of a super-resolution frame (correct_motion_fast)


def test_super_resolution_frames_fit_the_band_limited_transforms():
    """8184 x 11520 (BASELINE config 5 frames): the rows (5760 = 2^7 3^2 5 complex points) and the
    columns (8184 = 2^3 3 11 31: radix-31 and radix-11 passes) are transformed directly by the
    mixed-radix engine (round 2; chirp-z lines of 8192 / 16384 points before)."""
    low, high = plan.band_limits((300, 10), 1.0)
    g = plan.xc_geometry(8184, 11520, high, 8184 / 4, 8184 / 8)
    assert (g.nkx, g.kyp + g.kyn) == (1153, 1637) and g.RG >= 1 and 8184 % g.RG == 0
    fwd, _ = plan.line_plan(5760, -1, "cpu", keep=g.nkx + 1)
    inv, _ = plan.line_plan(5760, +1, "cpu")
    col, _ = plan.line_plan(8184, -1, "cpu")
    assert (fwd.M, fwd.keep, inv.M, col.M) == (5760, 0, 5760, 8184)
    col4, _ = plan.line_plan(4092, +1, "cpu")
    assert (col4.M, col4.keep) == (4092, 0)
    try:  # the chirp-z plans are still there (other lengths, and as the cross-check of the direct lines)
        plan.USE_DIRECT_LINES = False
        plan._LINES.clear()
        fwd, _ = plan.line_plan(5760, -1, "cpu", keep=g.nkx + 1)
        inv, _ = plan.line_plan(5760, +1, "cpu")
        col, _ = plan.line_plan(8184, -1, "cpu")
        col4, _ = plan.line_plan(4092, +1, "cpu")
        assert (fwd.M, fwd.keep, inv.M, col.M, col4.M) == (8192, g.nkx + 1, 16384, 16384, 8192)
    finally:
        plan.USE_DIRECT_LINES = True
        plan._LINES.clear()
    assert 8 * (plan.bluestein_size(5760) * 17 // 16 + 1 + g.nkx * (g.RG + 1)) <= 160 * 1024


def test_k3_geometry_and_chirp_tables():
    """BASELINE config 3 frames (4092 x 5760) go through the chirp-z path."""
    low, high = plan.band_limits((300, 10), 1.0)
    g = plan.xc_geometry(4092, 5760, high, 1023.0, 511.5)
    assert (g.nkx, g.kyp, g.kyn) == (577, 410, 409) and 4092 % g.RG == 0 and g.ny % g.RG == 0
    line, (tw, chirp, bspec) = plan.line_plan(12, -1, "cpu")
    assert line.M == 32 and chirp.shape == (12, 2) and bspec.shape == (32, 2)
    # chirp-z identity on the host: DFT_12(x) == c * ifft(fft(x*c, 32) * B)[:12] * 32 (B holds 1/32)
    rng = np.random.default_rng(0)
    x = rng.standard_normal(12) + 1j * rng.standard_normal(12)
    c = chirp.numpy()[:, 0] + 1j * chirp.numpy()[:, 1]
    B = bspec.numpy()[:, 0] + 1j * bspec.numpy()[:, 1]
    a = np.zeros(32, complex)
    a[:12] = x * c
    X = c * (np.fft.ifft(np.fft.fft(a) * B) * 32)[:12]
    assert np.allclose(X, np.fft.fft(x), atol=1e-5)


def test_band_limits_follow_reference_ops():
    low, high = plan.band_limits((300, 10), 1.0)
    assert low == pytest.approx(1 / 300, rel=1e-6) and high == pytest.approx(0.1, rel=1e-6)
    assert np.float32(high) == np.float32(torch.as_tensor(1 / torch.tensor(10.0)) * 1.0)


def test_twiddles():
    tw = plan.twiddles(8, "cpu").numpy()
    k = np.arange(8)
    assert np.allclose(tw[:, 0], np.cos(2 * np.pi * k / 8), atol=1e-7)
    assert np.allclose(tw[:, 1], -np.sin(2 * np.pi * k / 8), atol=1e-7)


# ------------------------------------------------------------------ spline taps


@pytest.mark.parametrize("kind", ["catmull_rom", "bspline"])
@pytest.mark.parametrize("shape", [(4, 3, 5), (5, 1, 1), (2, 2, 2), (1, 1, 1), (6, 1, 4)])
def test_axis_taps_reproduce_oracle_spline(kind, shape):
    g = torch.Generator().manual_seed(3)
    data = torch.randn(2, *shape, generator=g)
    ut, uy, ux = torch.linspace(0, 1, 7), torch.rand(5, generator=g), torch.linspace(0, 1, 6)
    taps = [spline.axis_taps(n, u, kind) for n, u in zip(shape, (ut, uy, ux))]
    out = torch.zeros(2, 7, 5, 6)
    for it in range(7):
        for iy in range(5):
            for ix in range(6):
                acc = torch.zeros(2)
                for kt in range(4):
                    for ky in range(4):
                        for kx in range(4):
                            w = taps[0][1][it, kt] * taps[1][1][iy, ky] * taps[2][1][ix, kx]
                            acc += w * data[:, taps[0][0][it, kt], taps[1][0][iy, ky], taps[2][0][ix, kx]]
                out[:, it, iy, ix] = acc
    tyx = torch.stack(torch.meshgrid(ut, uy, ux, indexing="ij"), -1)
    ref = tp.cubic_spline_grid_3d(data, tyx, kind).permute(3, 0, 1, 2)
    assert torch.allclose(out, ref, atol=2e-5)


def test_axis_taps_bad_kind():
    with pytest.raises(ValueError, match="grid_type"):
        spline.axis_taps(4, torch.linspace(0, 1, 3), "linear")


# ------------------------------------------------------------------ C ABI


def test_library_exports_every_declared_symbol():
    declared = declared_entry_points()
    assert len(declared) >= 20
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.mc_abi_version() == 1


def test_abi_rejects_bad_arguments_without_touching_the_gpu():
    lib = _lib.load()
    g = plan.xc_geometry(64, 64, 0.1, 16, 8)
    assert lib.mc_xc_rows_lds_bytes(g) > 0
    bad = _lib.XcGeom(W=100, H=64, nkx=5, kyp=5, kyn=4, y0=0, ny=64, x0=0, x1=100, RG=16)
    assert lib.mc_xc_rows_lds_bytes(bad) == -2  # MC_ERR_UNSUPPORTED: not a power of two
    n = ctypes.c_int64(0)
    assert lib.mc_warp_scratch_bytes(4, 64, 64, 10, 10, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.mc_warp_rigid_scratch_bytes(4, 64, 64, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.mc_circle_mask(None, None, 64, 64, 16.0, 8.0, None) == -1  # MC_ERR_ARG
    assert lib.mc_warp_frames_t(None, 3, 1, 64, 64, None, 10, 10, 1.0, None, None, None, None) == -1


def test_full_spectrum_and_storage_entry_points_check_arguments_on_the_host():
    """The round-2 entry points (row-major full-spectrum transforms, fp16 storage tags) check sizes,
    pointers and storage tags before any launch: pitch rule, supported row / column lengths (powers of
    two and the K3 formats), MC_ERR_ARG for null pointers, MC_ERR_UNSUPPORTED for sizes the library has
    no kernel for and for storage types that are not read natively."""
    lib = _lib.load()
    one = ctypes.c_void_p(16)  # a non-null, 16-byte aligned address: argument checks never dereference it
    assert [lib.mc_full_spectrum_pitch(w) for w in (64, 4096, 5760, 11520)] == [48, 2064, 2896, 5776]
    for (h, w) in ((4096, 4096), (256, 64), (4092, 5760), (8184, 11520), (4092, 4096), (256, 11520)):
        pitch = lib.mc_full_spectrum_pitch(w)
        assert lib.mc_full_rows_forward(None, one, w, one, one, 1, h, w, pitch, None) == -1  # null src
        assert lib.mc_full_cols_shift(None, one, one, 1.0, 1, h, w, pitch, None) == -1
        assert lib.mc_full_rows_inverse(one, None, one, w, one, 1, h, w, pitch, None) == -1
        assert lib.mc_full_cols_shift_sum(one, None, 0, 0, 1, one, None, one, h, w, pitch, 1.0, 0.0, 1.0, 300.0, 1,
                                          1, 1.0, None) == -1
    for (h, w) in ((4000, 4096), (4096, 4000), (128, 64), (8192, 64), (4092, 32)):  # no kernel for these
        pitch = lib.mc_full_spectrum_pitch(w)
        assert lib.mc_full_rows_forward(one, one, w, one, one, 1, h, w, pitch, None) == -2
        assert lib.mc_full_cols_shift(one, one, one, 1.0, 1, h, w, pitch, None) == -2
    assert lib.mc_full_rows_forward(one, one, 4096, one, one, 1, 4096, 4096, 2049, None) == -2  # pitch rule
    # storage tags: 2 = fp16, 3 = fp32 are read natively; raw detector types go through mc_condition_movie
    n = ctypes.c_int64(0)
    assert lib.mc_warp_rigid_scratch_bytes(2, 64, 64, ctypes.byref(n)) == 0
    assert lib.mc_warp_rigid_phase_t(one, 0, 2, 64, 64, one, one, one, one, 0, None) == -2   # u8 frames
    assert lib.mc_warp_rigid_phase_t(one, 2, 2, 64, 60, one, one, one, one, 0, None) == -2   # fp16, w % 8 != 0
    assert lib.mc_warp_rigid_phase_t(one, 3, 2, 64, 64, None, one, one, one, 0, None) == -1  # null shifts
    assert lib.mc_xc_provisional_mean_t(one, 1, 16, one, None) == -2 and lib.mc_xc_provisional_mean_t(None, 2, 16, one, None) == -1
    g = plan.xc_geometry(4096, 4096, 0.1, 1024, 512)
    assert lib.mc_xc_rows_forward_stats_t(one, 1, one, 4096, one, one, one, one, 1, g, 1024, 3072, 1024, 3072, one,
                                          one, one, None, None) == -2  # int16 frames are not read natively


def test_fp16_stacks_never_reach_an_fp32_only_kernel():
    """fp16 storage is read natively by the LDS-staged kernels only; every other shape must come back as
    MC_ERR_UNSUPPORTED *before* any launch (the callers then widen once), never fall through to a kernel
    that would read the 16-bit buffer as fp32 -- twice its bytes.  Checked on the host with
    pointers that are never dereferenced: rows that are not whole 8-sample units, an unaligned stack, a
    dense (per-pixel) lattice; and the rigid warp the same way."""
    lib = _lib.load()
    fake = lambda a: ctypes.c_void_p(a)  # noqa: E731  (never dereferenced: the shape checks come first)
    F16, F32 = 2, 3
    ok_ptr, odd_ptr = 0x10000, 0x10004
    cases = [
        (ok_ptr, 4, 64, 68, 10, 10),    # w % 8 != 0 (but w % 4 == 0: the fp32 tile kernels would take it)
        (ok_ptr, 4, 64, 66, 10, 10),    # w % 4 != 0: the untiled fp32 kernel's shape
        (odd_ptr, 4, 64, 64, 10, 10),   # stack not 16-byte aligned
        (ok_ptr, 4, 64, 64, 64, 64),    # dense lattice: warp_field2's case, fp32 only
    ]
    for base, t, h, w, GH, GW in cases:
        rc = lib.mc_warp_frames_t(fake(base), F16, t, h, w, fake(0x20000), GH, GW, 1.0, fake(0x30000), fake(0x40000),
                                  None, None)
        assert rc == -2, (base, t, h, w, GH, GW, rc)
    # storage tags that no warp reads natively
    for tag in (0, 1, 7):
        assert lib.mc_warp_frames_t(fake(ok_ptr), tag, 4, 64, 64, fake(0x20000), 10, 10, 1.0, fake(0x30000),
                                    fake(0x40000), None, None) == -2
    for base, w in ((ok_ptr, 68), (odd_ptr, 64)):
        assert lib.mc_warp_rigid_phase_t(fake(base), F16, 4, 64, w, fake(0x20000), fake(0x30000), fake(0x40000),
                                         None, 0, None) == -2
    header = open(os.path.join(ROOT, "include", "mcorr.h")).read()
    assert "#define MC_STORE_F16 2" in header and "#define MC_STORE_F32 3" in header and F32 == 3


def test_field_warp_entry_points_reject_in_a_fixed_order():
    """The return code of mc_warp_frames_t and mc_warp_frames_raw for inputs that reach each early return, with
    pointers that are never dereferenced (no case gets as far as a launch).  What matters is the ORDER of the
    checks where an input fails two of them: for fp16 storage the shape checks (w % 8, alignment, lattice density)
    come before the null-pointer checks, so an unsupported shape with a null lattice is -2 (MC_ERR_UNSUPPORTED),
    not -1 (MC_ERR_ARG) -- except a frame beyond 32-bit offsets, which is refused after them; for raw storage
    every argument check comes before every shape check.  The expected codes were taken by running this test
    against the library as it was before the route decision moved into one function (field_route, warp_field.hip):
    it passed there unchanged."""
    lib = _lib.load()
    fake = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
    U8, I16, F16, F32 = 0, 1, 2, 3
    FR, LAT, SCR, OUT, GAIN, MU = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000

    def warp_t(storage, frames=FR, t=4, h=256, w=64, lattice=LAT, GH=10, GW=10, ps=1.0, scratch=SCR, out=OUT, out_sum=0):
        return lib.mc_warp_frames_t(fake(frames), storage, t, h, w, fake(lattice), GH, GW, ps, fake(scratch), fake(out),
                                    fake(out_sum), None)

    for tag in (U8, I16, 7, -1):  # a bad storage tag wins over everything, null pointers included
        assert warp_t(tag) == -2 and warp_t(tag, frames=0, lattice=0, scratch=0, out=0) == -2
    fp16_shapes = [dict(w=68), dict(w=66), dict(frames=FR + 4), dict(frames=FR + 8), dict(GH=64, GW=64), dict(h=193, GH=11)]
    for shape in fp16_shapes:  # fp16: the shape first ...
        assert warp_t(F16, **shape) == -2, shape
        assert warp_t(F16, lattice=0, **shape) == -2, shape
        assert warp_t(F16, lattice=0, scratch=0, out=0, t=0, **shape) == -2, shape
    assert warp_t(F16, h=193, lattice=0) == -1 and warp_t(F16, h=192, lattice=0) == -2  # 64 (GH - 1) <= 3 (h - 1), GH = 10
    assert warp_t(F32, h=1) == -1 and warp_t(F16, h=1) == -2 and warp_t(F16, h=1, GH=1) == -1  # one row is a dense lattice
    assert warp_t(F32, w=1) == -1 and warp_t(F16, w=1) == -2
    # ... but not the 32-bit offset rule: with a bad argument that frame is MC_ERR_ARG
    assert warp_t(F16, h=65536, w=32768, lattice=0) == -1 and warp_t(F16, h=65536, w=32768, out=0) == -1
    assert warp_t(F16, h=65536, w=32772, lattice=0) == -2  # w % 8 != 0 still comes first
    for storage in (F16, F32):
        for null in ("frames", "lattice", "scratch"):
            assert warp_t(storage, **{null: 0}) == -1, (storage, null)
        assert warp_t(storage, out=0, out_sum=0) == -1  # no output requested
        for bad in (dict(t=0), dict(w=0), dict(GH=0), dict(GW=0), dict(ps=0.0), dict(ps=-1.0),
                    dict(ps=float("nan"))):
            assert warp_t(storage, **bad) == -1, (storage, bad)
        assert warp_t(storage, scratch=SCR + 4) == -1 and warp_t(storage, scratch=SCR + 8) == -1  # misaligned scratch
    # fp32 shapes that only a fallback kernel takes are no error: with a bad argument they are MC_ERR_ARG
    for shape in (dict(w=66), dict(frames=FR + 4), dict(GH=64, GW=64), dict(h=65536, w=32768)):
        assert warp_t(F32, lattice=0, **shape) == -1, shape

    def warp_raw(storage, raw=FR, gain=GAIN, mu=MU, t=4, h=256, w=64, lattice=LAT, GH=10, GW=10, ps=1.0, scratch=SCR,
                 out=OUT, out_sum=0, entry=lib.mc_warp_frames_raw):
        return entry(fake(raw), storage, fake(gain), fake(mu), t, h, w, fake(lattice), GH, GW, ps, fake(scratch),
                     fake(out), fake(out_sum), None)

    for tag in (F16, F32, 7, -1):
        assert warp_raw(tag) == -2 and warp_raw(tag, raw=0, lattice=0) == -2
    raw_shapes = {U8: [dict(w=72), dict(w=68)], I16: [dict(w=68), dict(w=66)]}  # raw w not a multiple of the unit
    for storage in (U8, I16):
        for null in ("raw", "gain", "mu", "lattice", "scratch"):
            assert warp_raw(storage, **{null: 0}) == -1, (storage, null)
        assert warp_raw(storage, out=0, out_sum=0) == -1
        for bad in (dict(t=0), dict(h=1), dict(w=0), dict(GH=0), dict(GW=0), dict(ps=0.0), dict(ps=float("nan"))):
            assert warp_raw(storage, **bad) == -1, (storage, bad)
        assert warp_raw(storage, scratch=SCR + 8) == -1
        shapes = raw_shapes[storage] + [dict(raw=FR + 8), dict(gain=GAIN + 2), dict(GH=64, GW=64),  # ... a dense lattice
                                        dict(h=65536, w=32768)]
        for shape in shapes:  # raw: every argument check first
            assert warp_raw(storage, **shape) == -2, (storage, shape)
            if "gain" not in shape:
                assert warp_raw(storage, gain=0, **shape) == -1, (storage, shape)
            assert warp_raw(storage, lattice=0, **shape) == -1 and warp_raw(storage, scratch=SCR + 4, **shape) == -1
        # the accumulating entry needs the sum, whatever else it is given
        acc = lib.mc_warp_frames_raw_accumulate
        assert warp_raw(storage, entry=acc) == -1 and warp_raw(storage, entry=acc, w=68, out_sum=OUT) == -2
        assert warp_raw(7, entry=acc) == -1 and warp_raw(7, entry=acc, out_sum=OUT) == -2


def test_rows_forward_entry_points_reject_in_a_fixed_order():
    """The return code of every early return that the entry points of K1 (forward row pass of the cross-correlation
    estimate, xc_rows_fwd.hip) reach before their first HIP call, with pointers that are never dereferenced: no
    case gets as far as a launch.  Inputs that fail two checks at once pin the ORDER: the storage tag comes before
    the geometry, the geometry before the pointers, the pointers before the shape and alignment rules of the
    1024-sample engine; mc_xc_provisional_mean_t alone looks at its pointers before the tag.  The route between
    the wave-per-row and the workgroup-per-row engine shows through a 4096-column geometry whose staging tile
    does not fit a CU's LDS: the workgroup engine refuses it (MC_ERR_ARG) before any HIP call, so every input that
    must NOT take the wave engine (a misaligned pointer, a row pitch that is no whole 16-byte unit, per-job
    exponents, no mask, mc_xc_row_engine(1)) comes back as -1.  The expected codes were taken by running this test
    against the library as it was when all three engines and the entry points were one source file: it passed
    there unchanged."""
    lib = _lib.load()
    fake = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
    ARG, UNS, OK = -1, -2, 0
    U8, I16, F16, F32 = 0, 1, 2, 3
    SRC, OFF, EXA, EXB, MASK, MR, T1, T1B, TW, GAIN, SUB = (0x10000 * (i + 1) for i in range(11))

    def geom(W=64, H=64, nkx=9, kyp=5, kyn=4, y0=0, ny=None, x0=0, x1=None, RG=16):
        return _lib.XcGeom(W=W, H=H, nkx=nkx, kyp=kyp, kyn=kyn, y0=y0, ny=H if ny is None else ny, x0=x0,
                           x1=W if x1 is None else x1, RG=RG)

    small = geom()
    patch = geom(W=1024, H=1024, nkx=100, kyp=10, kyn=10, RG=8)  # rows the 1024-sample engine takes
    # 4096-sample rows the wave engine takes; the workgroup engine's LDS would be 8 (2 * 2177 + 512 * 33) bytes
    big = geom(W=4096, H=4096, nkx=512, kyp=10, kyn=10, RG=32)
    assert 8 * (2 * 2177 + 512 * 33) > 160 * 1024
    # geom_from's own checks, in its order (sizes before counts), shared by every entry that converts a geometry
    bad_geoms = [(None, ARG), (geom(W=100), UNS), (geom(W=16, nkx=5), UNS), (geom(W=16384), UNS), (geom(H=1), UNS),
                 (geom(H=8200, RG=8), UNS), (geom(W=100, nkx=0), UNS), (geom(nkx=0), ARG), (geom(nkx=34), ARG),
                 (geom(kyp=0, kyn=0), ARG), (geom(kyp=60, kyn=5), ARG), (geom(RG=0), ARG), (geom(ny=60), ARG),
                 (geom(RG=2), ARG), (geom(y0=16), ARG), (geom(y0=-16, ny=16), ARG), (geom(x1=0), ARG),
                 (geom(x1=66), ARG), (geom(x0=1), ARG), (geom(x1=63), ARG)]

    # ---- mc_xc_rows_lds_bytes
    assert lib.mc_xc_rows_lds_bytes(small) == 8 * (4 * 2 * 35 + 9 * 17)  # four sub-groups of 32-point lines
    assert lib.mc_xc_rows_lds_bytes(big) == 8 * (2 * 2177 + 512 * 33)
    for q, code in bad_geoms:
        assert lib.mc_xc_rows_lds_bytes(q) == code, q and [getattr(q, n) for n, _ in q._fields_]

    # ---- mc_xc_rows_forward
    def fwd(src=SRC, off=OFF, stride=None, expo=0, mask=MASK, mr=MR, t1=T1, tw=TW, n=2, q=small):
        stride = q.W if stride is None and q else stride or 64
        return lib.mc_xc_rows_forward(fake(src), fake(off), stride, fake(expo), fake(mask), fake(mr), fake(t1), fake(tw),
                                      n, q, None)

    for q, code in bad_geoms:  # the geometry before the pointers
        assert fwd(q=q) == code and fwd(q=q, src=0, off=0, t1=0, tw=0, n=0) == code
    for null in ("src", "off", "t1", "tw", "n"):
        assert fwd(**{null: 0}) == ARG and fwd(q=big, **{null: 0}) == ARG, null
    assert fwd(n=-1) == ARG
    # the route: none of these may take the wave engine
    for wg in (dict(src=SRC + 4), dict(src=SRC + 8), dict(mask=MASK + 4), dict(mask=MASK + 8), dict(mask=0),
               dict(expo=EXA), dict(stride=4098), dict(stride=4097), dict(mr=0, mask=0)):
        assert fwd(q=big, **wg) == ARG, wg
    for q in (geom(W=4096, H=4096, nkx=600, kyp=10, kyn=10, RG=32),                 # more than 512 kept bins
              geom(W=4096, H=4096, nkx=512, kyp=10, kyn=10, ny=4092, RG=44),        # no whole rounds of 8 rows
              geom(W=2048, H=4096, nkx=512, kyp=10, kyn=10, RG=64),
              geom(W=8192, H=4096, nkx=512, kyp=10, kyn=10, RG=32)):
        assert fwd(q=q) == ARG, [getattr(q, n) for n, _ in q._fields_]

    # ---- mc_xc_row_engine
    assert lib.mc_xc_row_engine(-1) == ARG and lib.mc_xc_row_engine(2) == ARG
    try:
        assert lib.mc_xc_row_engine(1) == OK
        assert lib.mc_xc_row_engine(7) == ARG  # ... and the mode stays 1:
        assert fwd(q=big) == ARG               # rows the wave engine would take go to the workgroup engine
    finally:
        assert lib.mc_xc_row_engine(0) == OK

    # ---- mc_xc_rows_forward_raw
    def fwd_raw(storage, raw=SRC, gain=GAIN, off=OFF, stride=None, mask=MASK, sub=SUB, mr=MR, t1=T1, tw=TW, n=2, q=small):
        stride = q.W if stride is None and q else stride or 64
        return lib.mc_xc_rows_forward_raw(fake(raw), storage, fake(gain), fake(off), stride, fake(mask), fake(sub),
                                          fake(mr), fake(t1), fake(tw), n, q, None, None)

    raw_nulls = ("raw", "gain", "off", "mask", "sub", "mr", "t1", "tw", "n")
    for tag in (F16, F32, 7, -1):  # a bad storage tag wins over everything
        assert fwd_raw(tag) == UNS and fwd_raw(tag, q=None) == UNS and fwd_raw(tag, q=geom(nkx=0), raw=0, n=0) == UNS
    for storage in (U8, I16):
        for q, code in bad_geoms:
            assert fwd_raw(storage, q=q) == code and fwd_raw(storage, q=q, raw=0, gain=0, n=0) == code
        for null in raw_nulls:
            assert fwd_raw(storage, **{null: 0}) == ARG and fwd_raw(storage, q=big, **{null: 0}) == ARG, null
        # the route: 16-byte raw, gain and mask and a pitch of whole 8-sample units, or the workgroup engine
        for wg in (dict(raw=SRC + 8), dict(raw=SRC + 1), dict(gain=GAIN + 8), dict(gain=GAIN + 4), dict(mask=MASK + 8),
                   dict(stride=4100), dict(stride=4098)):
            assert fwd_raw(storage, q=big, **wg) == ARG, (storage, wg)
        assert fwd_raw(storage, q=geom(W=8192, H=4096, nkx=512, kyp=10, kyn=10, RG=32)) == ARG

    # ---- mc_xc_rows_forward_dual_t
    def dual(storage, src=SRC, off=OFF, stride=1024, exa=EXA, exb=EXB, mask=MASK, mr=MR, t1a=T1, t1b=T1B, tw=TW, n=2,
             q=patch):
        return lib.mc_xc_rows_forward_dual_t(fake(src), storage, fake(off), stride, fake(exa), fake(exb), fake(mask),
                                             fake(mr), fake(t1a), fake(t1b), fake(tw), n, q, None, None)

    not_patch_rows = [small, big, geom(W=512, H=1024, nkx=100, kyp=10, kyn=10, RG=8),
                      geom(W=2048, H=1024, nkx=100, kyp=10, kyn=10, RG=8),
                      geom(W=1024, H=1024, nkx=129, kyp=10, kyn=10, RG=8),
                      geom(W=1024, H=1024, nkx=100, kyp=10, kyn=10, ny=1020, RG=4)]
    dual_nulls = ("src", "off", "exa", "mask", "t1a", "tw", "n")
    for tag in (U8, I16, 7, -1):
        assert dual(tag) == UNS and dual(tag, q=None) == UNS and dual(tag, q=geom(nkx=0), src=0, n=0) == UNS
    for storage in (F16, F32):
        for q, code in bad_geoms:
            assert dual(storage, q=q) == code and dual(storage, q=q, src=0, mask=0, n=0) == code
        for null in dual_nulls:
            assert dual(storage, **{null: 0}) == ARG, null
            for q in not_patch_rows:  # a null pointer wins over a shape the engine does not take
                assert dual(storage, q=q, **{null: 0}) == ARG, null
            assert dual(storage, mask=MASK + 4, **({null: 0} if null != "mask" else {"src": 0})) == ARG
        assert dual(storage, t1b=0) == ARG and dual(storage, t1b=0, q=small) == ARG  # a second exponent without its T1
        assert dual(storage, n=-3) == ARG
        for q in not_patch_rows:
            assert dual(storage, q=q) == UNS and dual(storage, q=q, exb=0, t1b=0) == UNS
        assert dual(storage, mask=MASK + 4) == UNS and dual(storage, mask=MASK + 12) == UNS

    # ---- mc_xc_rows_forward_dual_raw
    def dual_raw(storage, raw=SRC, gain=GAIN, area=1 << 20, off=OFF, stride=1024, exa=EXA, exb=EXB, mask=MASK, sub=SUB,
                 mr=MR, t1a=T1, t1b=T1B, tw=TW, n=2, q=patch):
        return lib.mc_xc_rows_forward_dual_raw(fake(raw), storage, fake(gain), area, fake(off), stride, fake(exa),
                                               fake(exb), fake(mask), fake(sub), fake(mr), fake(t1a), fake(t1b),
                                               fake(tw), n, q, None, None)

    dual_raw_bad = [dict(raw=0), dict(gain=0), dict(off=0), dict(exa=0), dict(mask=0), dict(sub=0), dict(mr=0),
                    dict(t1a=0), dict(tw=0), dict(n=0), dict(t1b=0), dict(area=0), dict(stride=0), dict(stride=-1024)]
    for tag in (F16, F32, 7, -1):
        assert dual_raw(tag) == UNS and dual_raw(tag, q=None) == UNS and dual_raw(tag, q=geom(nkx=0), raw=0) == UNS
    for storage in (U8, I16):
        for q, code in bad_geoms:
            assert dual_raw(storage, q=q) == code and dual_raw(storage, q=q, raw=0, gain=0, area=0) == code
        for bad in dual_raw_bad:
            assert dual_raw(storage, **bad) == ARG, bad
            for q in not_patch_rows:
                assert dual_raw(storage, q=q, **bad) == ARG, bad
            if "gain" not in bad:  # ... and over the raw entry's own alignment rules
                assert dual_raw(storage, **{"gain": GAIN + 2, **bad}) == ARG, bad
        for q in not_patch_rows:
            assert dual_raw(storage, q=q) == UNS and dual_raw(storage, q=q, exb=0, t1b=0) == UNS
        assert dual_raw(storage, mask=MASK + 4) == UNS
        assert dual_raw(storage, gain=GAIN + 2) == UNS and dual_raw(storage, gain=GAIN + 1) == UNS
    assert dual_raw(I16, raw=SRC + 1) == UNS and dual_raw(I16, raw=SRC + 1, tw=0) == ARG  # (u8 rows may start anywhere)

    # ---- mc_xc_rows_forward_stats_t: the storage tag, the pointers it reads itself, then the box (it clears the
    # accumulators before it looks at anything else)
    def stats(storage, m0=MR, acc=SUB, fix=GAIN, out3=T1B, q=small, hl=16, hu=48, wl=16, wu=48):
        return lib.mc_xc_rows_forward_stats_t(fake(SRC), storage, fake(OFF), 64, fake(MASK), fake(m0), fake(T1), fake(TW),
                                              2, q, hl, hu, wl, wu, fake(acc), fake(fix), fake(out3), None, None)

    windowed = geom(y0=16, ny=32, x0=16, x1=48)
    boxes = [dict(hl=0), dict(hu=64), dict(wl=0), dict(wl=14), dict(wu=64), dict(wu=50), dict(wl=17), dict(wu=47),
             dict(hl=48), dict(hl=40, hu=32), dict(wl=48), dict(wl=40, wu=32)]
    for tag in (U8, I16, 7, -1):
        assert stats(tag) == UNS and stats(tag, m0=0, acc=0, q=None) == UNS and stats(tag, q=windowed, hl=0) == UNS
    for storage in (F16, F32):
        for null in ("m0", "acc", "fix", "out3"):
            assert stats(storage, **{null: 0}) == ARG and stats(storage, q=windowed, hl=0, **{null: 0}) == ARG, null
        assert stats(storage, q=None) == ARG
        for box in boxes:  # the box must lie inside the region K1 reads, on even columns, and hold something
            assert stats(storage, q=windowed, **box) == ARG, box
        assert stats(storage, q=geom(W=100, y0=16, ny=32, x0=16, x1=48), hl=0) == ARG  # the box before the geometry

    # ---- mc_xc_provisional_mean_t: the pointers and the count before the tag
    def pmean(storage, x=SRC, n=16, m0=MR):
        return lib.mc_xc_provisional_mean_t(fake(x), storage, n, fake(m0), None)

    for tag in (U8, I16, 7, -1):
        assert pmean(tag) == UNS
        assert pmean(tag, x=0) == ARG and pmean(tag, m0=0) == ARG and pmean(tag, n=0) == ARG and pmean(tag, n=-1) == ARG
    for storage in (F16, F32):
        assert pmean(storage, x=0) == ARG and pmean(storage, m0=0) == ARG and pmean(storage, n=0) == ARG

    # ---- mc_xc_rows_hot_correct
    def hot(keys=SRC, rv=OFF, n=0, frame0=0, njobs=2, h=64, w=64, mask=MASK, mr=MR, t1=T1, q=small):
        return lib.mc_xc_rows_hot_correct(fake(keys), fake(rv), n, frame0, njobs, h, w, fake(mask), fake(mr), fake(t1), q,
                                          None)

    assert hot() == OK and hot(mask=0) == OK  # an empty list is no work, and no error; the mask is optional
    for bad in (dict(keys=0), dict(rv=0), dict(mr=0), dict(t1=0), dict(q=None), dict(n=-1), dict(frame0=-1),
                dict(njobs=0), dict(h=0), dict(w=0), dict(w=128), dict(q=geom(W=128)), dict(q=geom(nkx=0)),
                dict(q=geom(ny=0)), dict(q=geom(y0=-16)), dict(q=geom(y0=16)), dict(h=32), dict(n=1 << 31)):
        assert hot(**bad) == ARG, bad  # ... but every argument is checked before the list is found empty
        if "n" not in bad:
            assert hot(n=5, **bad) == ARG, bad


def test_full_spectrum_and_generic_length_entry_points_reject_in_a_fixed_order():
    """The return code of every early return of the row-major full-spectrum entry points (full_fft.hip,
    full_sums.hip), of mc_xcg_rows_forward_raw and of the geometry and line checks of the generic-length engine
    (xcg_common.h, reached through mc_xcg_cols_forward), with pointers that are never dereferenced: no case gets
    as far as a launch.  Inputs that fail two checks at once pin the ORDER: arguments (MC_ERR_ARG, -1) come before
    sizes (MC_ERR_UNSUPPORTED, -2) in the full-spectrum entries, except that the raw row pass looks at `kind`
    between the two; the raw generic-length row pass looks at the storage tag first, then geometry, then the line,
    then the pointers, then the line code.  The expected codes were taken by running this test against the library
    as it was when full_fft.hip and xcg_fft.hip were each one file compiled several times under a macro: it passed
    there unchanged."""
    lib = _lib.load()
    fake = lambda a: ctypes.c_void_p(a) if a else None  # noqa: E731
    ARG, UNS, OK = -1, -2, 0
    A, B, C_, D, E, F = (0x10000 * (i + 1) for i in range(6))  # 16-byte aligned, never dereferenced
    good = dict(h=256, w=64, pitch=48)
    bad_sizes = [dict(h=4000), dict(h=128), dict(h=8192), dict(w=4000), dict(w=32), dict(w=16384), dict(pitch=49),
                 dict(pitch=32), dict(h=257)]

    def rows_fwd(src=A, off=B, stride=64, S=C_, tw=D, n=1, h=256, w=64, pitch=48):
        return lib.mc_full_rows_forward(fake(src), fake(off), stride, fake(S), fake(tw), n, h, w, pitch, None)

    def rows_inv(S=A, out=B, off=C_, stride=64, tw=D, n=1, h=256, w=64, pitch=48):
        return lib.mc_full_rows_inverse(fake(S), fake(out), fake(off), stride, fake(tw), n, h, w, pitch, None)

    def rows_raw(kind, raw=A, gain=B, mu=C_, off=D, S=E, tw=F, n=1, h=256, w=64, pitch=48):
        return lib.mc_full_rows_forward_raw(fake(raw), kind, fake(gain), fake(mu), fake(off), fake(S), fake(tw), n, h, w,
                                            pitch, None)

    def cols_shift(S=A, shifts=B, tw=C_, n=1, h=256, w=64, pitch=48):
        return lib.mc_full_cols_shift(fake(S), fake(shifts), fake(tw), 1.0, n, h, w, pitch, None)

    def transpose(S=A, ST=B, n=1, h=256, w=64, pitch=48):
        return lib.mc_full_transpose(fake(S), fake(ST), n, h, w, pitch, None)

    def hot(keys=A, rv=B, n=1, frame0=0, njobs=1, h=256, w=64, S=C_, pitch=48):
        return lib.mc_full_rows_hot_correct(fake(keys), fake(rv), n, frame0, njobs, h, w, fake(S), pitch, None)

    def sums(entry, S=A, shifts=B, nframes=2, frame0=0, total=2, acc=C_, plain=D, tw=E, h=256, w=64, pitch=48, ps=1.0,
             dose=1.0):
        return entry(fake(S), fake(shifts), nframes, frame0, total, fake(acc), fake(plain), fake(tw), h, w, pitch, ps,
                     0.0, dose, 300.0, 1, 1, 1.0, None)

    assert good == dict(h=256, w=64, pitch=lib.mc_full_spectrum_pitch(64))
    for entry, nulls in ((rows_fwd, ("src", "off", "S", "tw")), (rows_inv, ("S", "out", "off", "tw")),
                         (cols_shift, ("S", "shifts", "tw")), (transpose, ("S", "ST"))):
        for null in nulls:
            assert entry(**{null: 0}) == ARG, (entry.__name__, null)
            assert entry(h=4000, **{null: 0}) == ARG, (entry.__name__, null)  # null pointer + unsupported size
        assert entry(n=0) == ARG and entry(n=0, w=4000) == ARG and entry(n=-1, pitch=49) == ARG
        for size in bad_sizes:
            assert entry(**size) == UNS, (entry.__name__, size)
    assert rows_fwd(src=A + 4) == UNS and rows_fwd(stride=65) == UNS and rows_fwd(src=A + 4, S=0) == ARG
    assert rows_inv(out=B + 4) == UNS and rows_inv(stride=65) == UNS and rows_inv(out=B + 4, tw=0) == ARG
    # the raw row pass: pointers, then the kind, then sizes and alignment (u8 pairs: 2 bytes, i16 pairs: 4, gain: 8)
    for kind in (0, 1):
        for null in ("raw", "gain", "mu", "off", "S", "tw"):
            assert rows_raw(kind, **{null: 0}) == ARG and rows_raw(kind, h=4000, **{null: 0}) == ARG, (kind, null)
        assert rows_raw(kind, n=0) == ARG
        for size in bad_sizes:
            assert rows_raw(kind, **size) == UNS, (kind, size)
        assert rows_raw(kind, raw=A + 1) == UNS and rows_raw(kind, gain=B + 4) == UNS
    assert rows_raw(1, raw=A + 2) == UNS
    for kind in (2, 3, 4, -1):
        assert rows_raw(kind) == UNS and rows_raw(kind, h=4000) == UNS
        assert rows_raw(kind, gain=0) == ARG and rows_raw(kind, n=0) == ARG  # bad kind + null pointer
    # the hot-pixel fix: arguments, sizes and the alignment of rv, and only then "nothing to do"
    assert hot(n=0) == OK and hot(n=0, keys=0, rv=0) == OK
    assert hot(n=0, h=4000) == UNS and hot(n=0, rv=B + 4) == UNS and hot(n=0, pitch=49) == UNS
    assert hot(n=0, S=0) == ARG and hot(n=0, S=0, h=4000) == ARG and hot(n=0, njobs=0) == ARG and hot(n=0, frame0=-1) == ARG
    assert hot(n=-1) == ARG and hot(n=1 << 31) == ARG and hot(n=1 << 31, h=4000) == ARG
    assert hot(keys=0) == ARG and hot(rv=0) == ARG and hot(rv=0, w=4000) == ARG and hot(h=0) == ARG and hot(w=1) == ARG
    assert hot(h=4000) == UNS and hot(rv=B + 4) == UNS
    # the fused sums, row-major and column-major
    for entry in (lib.mc_full_cols_shift_sum, lib.mc_full_cols_shift_sum_cm):
        for bad in (dict(S=0), dict(acc=0, plain=0), dict(tw=0), dict(nframes=0), dict(frame0=-1), dict(total=1),
                    dict(frame0=1), dict(shifts=0), dict(shifts=0, acc=0), dict(ps=0.0), dict(ps=-1.0),
                    dict(ps=float("nan")), dict(dose=-1.0), dict(dose=float("nan")), dict(ps=0.0, plain=0)):
            assert sums(entry, **bad) == ARG, bad
            assert sums(entry, h=4000, **bad) == ARG, bad  # ... each of them before the sizes
        for size in bad_sizes:
            assert sums(entry, **size) == UNS, size
            assert sums(entry, ps=0.0, acc=0, **size) == UNS, size  # the plain sum alone has no pixel size to check
    for h in (256, 512, 1024, 2048):  # column-major copies: only for the columns that are read from one
        assert sums(lib.mc_full_cols_shift_sum_cm, h=h) == UNS and sums(lib.mc_full_cols_shift_sum_cm, h=h, plain=0) == UNS
        assert sums(lib.mc_full_cols_shift_sum_cm, h=h, shifts=0) == ARG  # P without shifts comes first
        assert sums(lib.mc_full_cols_shift_sum_cm, h=h, ps=0.0) == ARG
        assert sums(lib.mc_full_cols_shift_sum_cm, h=h, pitch=49) == UNS

    # ---- the generic-length engine: geom_from_g, then line_from, then the entry's own pointers
    def geom(**kw):
        f = dict(W=5760, H=4092, nkx=100, kyp=50, kyn=50, y0=0, ny=4092, x0=0, x1=5760, RG=4)
        f.update(kw)
        return _lib.XcGeom(**f)

    def line(M, keep=0, tw_m=A, chirp=B, bspec=C_):
        return _lib.XcLine(tw_m, chirp, bspec, M, keep)

    def cols_fwd(g=geom(), ln=line(4092), T1=D, S=E, n=1):
        return lib.mc_xcg_cols_forward(fake(T1), None, fake(S), ln, n, g, None)

    assert cols_fwd(g=None) == ARG and cols_fwd(g=None, ln=None) == ARG
    for size in (dict(W=3), dict(W=16386), dict(W=8193), dict(H=1), dict(H=8193)):
        assert cols_fwd(g=geom(**size)) == UNS, size
        assert cols_fwd(g=geom(nkx=0, **size)) == UNS and cols_fwd(g=geom(**size), ln=None, T1=0) == UNS, size
    for bad in (dict(nkx=0), dict(nkx=2882), dict(kyp=-1), dict(kyn=-1), dict(kyp=0, kyn=0), dict(kyp=4092, kyn=1),
                dict(RG=0), dict(ny=0), dict(ny=4090), dict(RG=5, ny=4090), dict(y0=-4), dict(y0=4), dict(x0=-2),
                dict(x1=5762), dict(x0=100, x1=100), dict(x0=1), dict(x1=5759)):
        assert cols_fwd(g=geom(**bad)) == ARG, bad
        assert cols_fwd(g=geom(**bad), ln=line(3000)) == ARG, bad  # the geometry before the line
    assert cols_fwd(ln=None) == ARG and cols_fwd(ln=None, T1=0) == ARG
    for null in ("tw_m", "chirp", "bspec"):
        assert cols_fwd(ln=line(4092, **{null: 0})) == ARG and cols_fwd(ln=line(3000, **{null: 0})) == ARG, null
    for M in (3000, 16, 32768, 5120 * 3):  # no line engine for M, or M outside 32 .. 16384
        assert cols_fwd(ln=line(M)) == UNS and cols_fwd(ln=line(M), T1=0) == UNS and cols_fwd(ln=line(M, keep=-1)) == UNS, M
    assert cols_fwd(ln=line(8192, keep=-1)) == ARG and cols_fwd(ln=line(8192, keep=8)) == ARG  # columns take no pruned plan
    assert cols_fwd(ln=line(4096)) == UNS and cols_fwd(ln=line(4096), T1=0) == UNS  # chirp-z needs M >= 2 n - 1
    assert cols_fwd(ln=line(8192, keep=8, chirp=0)) == ARG
    for ln in (line(4092), line(8192)):  # a direct and a chirp-z plan that pass: the entry's pointers are next
        assert cols_fwd(ln=ln, T1=0) == ARG and cols_fwd(ln=ln, S=0) == ARG and cols_fwd(ln=ln, n=0) == ARG

    U8, I16, F16, F32 = 0, 1, 2, 3

    def xcg_raw(storage, g=geom(), ln=line(2880), raw=A, gain=B, off=C_, mask=D, sub=E, mr=F, T1=A + 64, tw=B + 64, n=1):
        return lib.mc_xcg_rows_forward_raw(fake(raw), storage, fake(gain), fake(off), 5760, fake(mask), fake(sub),
                                           fake(mr), fake(T1), fake(tw), ln, n, g, None)

    for tag in (F16, F32, 7, -1):  # the storage tag before everything, a missing geometry included
        assert xcg_raw(tag) == UNS and xcg_raw(tag, g=None) == UNS and xcg_raw(tag, raw=0, ln=None) == UNS
    for st in (U8, I16):
        assert xcg_raw(st, g=None) == ARG and xcg_raw(st, g=geom(W=3)) == UNS and xcg_raw(st, g=geom(nkx=0)) == ARG
        odd = geom(W=5761, x1=5761)
        assert xcg_raw(st, g=odd) == UNS and xcg_raw(st, g=odd, ln=None) == UNS and xcg_raw(st, g=odd, raw=0) == UNS
        assert xcg_raw(st, ln=None) == ARG and xcg_raw(st, ln=line(3000)) == UNS and xcg_raw(st, ln=line(3000), raw=0) == UNS
        assert xcg_raw(st, ln=line(8192, keep=100)) == ARG  # a pruned plan must keep nkx + 1 outputs
        assert xcg_raw(st, ln=line(2048, keep=101)) == ARG  # ... in M >= n + 2 keep - 1 points
        for null in ("raw", "gain", "off", "mask", "sub", "mr", "T1", "tw"):
            assert xcg_raw(st, **{null: 0}) == ARG, (st, null)
        assert xcg_raw(st, n=0) == ARG
        # a line code other than 22 / 23 (direct 2880 / 5760 points): chirp-z plans, the direct column lengths
        others = [(geom(), line(8192)), (geom(), line(8192, keep=101)), (geom(W=8184, x1=8184), line(4092)),
                  (geom(W=16368, x1=16368), line(8184)), (geom(W=1000, x1=1000), line(1024))]
        for g, ln in others:
            assert xcg_raw(st, g=g, ln=ln) == UNS, (st, g.W, ln.M, ln.keep)
            assert xcg_raw(st, g=g, ln=ln, raw=0) == ARG and xcg_raw(st, g=g, ln=ln, n=0) == ARG  # the pointers first
        # the staging tile beyond a CU's LDS: the last check, and an argument error
        big = geom(W=11520, H=8184, nkx=2881, ny=8184, x1=11520, RG=6)
        assert xcg_raw(st, g=big, ln=line(5760)) == ARG and xcg_raw(st, g=big, ln=line(5760), raw=0) == ARG


def test_raw_entry_points_validate_on_the_host():
    """N2 entry points (mc_raw_movie_stats, mc_xc_rows_forward_raw, mc_warp_rigid_raw) check storage tags,
    shapes and pointers before any launch."""
    lib = _lib.load()
    fake = lambda a: ctypes.c_void_p(a)  # noqa: E731
    U8, I16, F16, F32 = 0, 1, 2, 3
    p = [fake(0x10000 * (i + 1)) for i in range(8)]
    # statistics: box must lie inside the frame; storage tag 0..3
    assert lib.mc_raw_movie_stats(p[0], U8, p[1], 4, 64, 64, 16, 48, 16, 80, 1, p[2], p[3], p[4], p[5], None) == -1
    assert lib.mc_raw_movie_stats(p[0], 9, p[1], 4, 64, 64, 16, 48, 16, 48, 1, p[2], p[3], p[4], p[5], None) == -2
    assert lib.mc_raw_movie_stats(None, U8, p[1], 4, 64, 64, 16, 48, 16, 48, 1, p[2], p[3], p[4], p[5], None) == -1
    # K1 from raw bytes: u8 / i16 only, power-of-two widths only (the K3 formats have mc_xcg_rows_forward_raw)
    g4096 = plan.xc_geometry(4096, 4096, 0.1, 16, 8)
    gk3 = plan.xc_geometry(4092, 5760, 0.1, 16, 8)
    args = lambda st, g: (p[0], st, p[1], p[2], 4096, p[3], p[4], p[5], p[6], p[7], 2, g, None, None)  # noqa: E731
    assert lib.mc_xc_rows_forward_raw(*args(F32, g4096)) == -2
    assert lib.mc_xc_rows_forward_raw(*args(F16, g4096)) == -2
    assert lib.mc_xc_rows_forward_raw(*args(U8, gk3)) in (-1, -2)
    assert lib.mc_xc_rows_forward_raw(None, U8, p[1], p[2], 4096, p[3], p[4], p[5], p[6], p[7], 2, g4096, None, None) == -1
    # rigid warp from raw bytes: rows of whole quads, aligned buffers, at most 256 frames
    w = lambda st, nf, ww, raw=p[0]: lib.mc_warp_rigid_raw(raw, st, p[1], p[2], nf, 64, ww, p[3], p[4], p[5], None,  # noqa: E731
                                                           0, None)
    assert w(F32, 4, 64) == -2 and w(F16, 4, 64) == -2
    assert w(U8, 4, 66) == -2 and w(U8, 300, 64) == -2 and w(I16, 4, 64, fake(0x10004)) == -2
    assert lib.mc_warp_rigid_raw(p[0], U8, None, p[2], 4, 64, 64, p[3], p[4], p[5], None, 0, None) == -1


def test_storage_kind_entries_keep_their_order_of_argument_checks():
    """The four entries that dispatch over the storage kind (u8, i16, f16, f32) return, for a kind outside
    0..3 and for null pointers, the codes their argument checks have always returned, in the same order:
    the two `condition` entries test the kind together with the pointers (MC_ERR_ARG), the two `raw_`
    entries test the pointers first (MC_ERR_ARG), then the kind (MC_ERR_UNSUPPORTED: the caller falls
    back), then the box (MC_ERR_ARG).  Every call ends in a check: nothing is launched."""
    lib = _lib.load()
    ARG, UNSUPPORTED = -1, -2
    p = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]  # aligned, never dereferenced
    box, off_box = (16, 48, 16, 48), (16, 80, 16, 48)

    def cond(kind, raw=p[0], out=p[3], t=4, hw=4096, mean_zero=1, sums=p[2]):
        return lib.mc_condition_movie(raw, kind, p[1], t, hw, mean_zero, sums, out, None)

    def cond_hot(kind, raw=p[0], thr=10.0, stats=p[2], out=p[4]):
        return lib.mc_condition_movie_hot(raw, kind, p[1], 4, 64, 64, 1, thr, stats, p[3], out, None)

    def stats(kind, raw=p[0], b=box, st=p[2], mu=p[3], sub=p[4], mr=p[5], t=4):
        return lib.mc_raw_movie_stats(raw, kind, p[1], t, 64, 64, *b, 1, st, mu, sub, mr, None)

    def detect(kind, raw=p[0], gain=p[1], b=box, w=64, keys=p[4], cap=100):
        return lib.mc_raw_hot_detect(raw, kind, gain, 4, 64, w, *b, 10.0, p[2], p[3], keys, p[5], cap, p[6], p[7],
                                     None)

    for kind in (-1, 4):
        assert cond(kind) == ARG and cond_hot(kind) == ARG, kind
        assert stats(kind) == UNSUPPORTED and detect(kind) == UNSUPPORTED, kind
        # pointers before the kind, the kind before the box and before the shape
        assert stats(kind, raw=None) == ARG and detect(kind, gain=None) == ARG, kind
        assert stats(kind, b=off_box) == UNSUPPORTED and detect(kind, b=off_box) == UNSUPPORTED, kind
        assert detect(kind, w=60) == UNSUPPORTED, kind
    for kind in (0, 1, 2, 3):
        assert cond(kind, raw=None) == ARG and cond(kind, out=None) == ARG and cond(kind, sums=None) == ARG
        assert cond(kind, t=0) == ARG and cond(kind, hw=0) == ARG
        assert cond_hot(kind, raw=None) == ARG and cond_hot(kind, out=None) == ARG and cond_hot(kind, stats=None) == ARG
        assert cond_hot(kind, thr=0.0) == ARG and cond_hot(kind, thr=float("nan")) == ARG
        assert stats(kind, raw=None) == ARG and stats(kind, st=None) == ARG and stats(kind, mu=None) == ARG
        assert stats(kind, sub=None) == ARG and stats(kind, mr=None) == ARG and stats(kind, t=0) == ARG
        assert stats(kind, b=off_box) == ARG
        assert detect(kind, raw=None) == ARG and detect(kind, gain=None) == ARG and detect(kind, keys=None) == ARG
        assert detect(kind, cap=0) == ARG and detect(kind, b=off_box) == ARG
        assert detect(kind, w=60) == UNSUPPORTED  # rows of whole 8-sample groups only
        # u8 samples are read 8 bytes at a time, every other kind 16
        assert detect(kind, raw=ctypes.c_void_p(0x10004 if kind == 0 else 0x10008)) == UNSUPPORTED


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "torch_motion_correction_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), fn


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import torch_motion_correction_amd as mc

    with pytest.raises(mc.McorrError, match="no CPU fallback"):
        mc.estimate_global_motion(torch.zeros(3, 64, 64), 1.0)


# ------------------------------------------------------------------ sharding (gloo, 2 ranks)


def test_round_robin_assignment():
    a = multi_gpu.assignment(64, 8)
    assert all(len(x) == 8 for x in a)
    assert sorted(i for x in a for i in x) == list(range(64))
    assert multi_gpu.movies_for_rank(5, 1, 2) == [1, 3]
    assert multi_gpu.movies_for_rank(1, 1, 2) == []  # ragged: more ranks than movies
    with pytest.raises(ValueError):
        multi_gpu.movies_for_rank(4, 2, 2)


def _rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        n_movies = 5
        mine = multi_gpu.movies_for_rank(n_movies, rank, world)
        # a CPU stand-in for the per-movie work: each movie's known integer drift is
        # "estimated" from its id alone, so the gathered table can be checked exactly
        local = multi_gpu.process_shard(mine, load=lambda i: torch.full((2,), float(i)),
                                        work=lambda x: (x * 2).tolist())
        dist.barrier()
        merged = multi_gpu.gather_results(local, world)
        elapsed = torch.tensor([0.1 * (rank + 1)], dtype=torch.float64)
        dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)  # the bench's max-over-ranks
        q.put((rank, mine, merged, float(elapsed)))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_sharding():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    results.sort()
    assert results[0][1] == [0, 2, 4] and results[1][1] == [1, 3]
    for _, _, merged, elapsed in results:
        assert merged == {i: [2.0 * i, 2.0 * i] for i in range(5)}
        assert elapsed == pytest.approx(0.2)


@pytest.mark.parametrize("t", [5, 40, 51, 60])
def test_leave_one_out_schedule_replays_the_table(t):
    """the incremental add/rebuild schedule must reproduce S_f exactly, the way the kernel
    applies it (rebuild: replace; otherwise: union)"""
    ref_expo, _, _ = lattice.mask_schedule(t, "mean_except_current", t // 2)
    ptr, idx, rebuild = lattice.leave_one_out_schedule(ref_expo)
    running: set = set()
    for f in range(t):
        lst = set(idx[ptr[f]:ptr[f + 1]].tolist()) if ptr[f + 1] > ptr[f] else set()
        running = lst if rebuild[f] else running | lst
        assert running == {o for o in range(t) if o != f and ref_expo[f, o] == 1}
    if t <= 50:
        assert int(rebuild.sum()) == 1  # only frame 0; afterwards one frame joins per step


def test_movie_pipeline_needs_a_gpu_and_is_exported():
    """No CPU fallback for the batch entry point either."""
    import torch_motion_correction_amd as m

    assert {"motion_correct_movies", "MoviePipeline", "MovieResult"} <= set(m.__all__)
    if not torch.cuda.is_available():
        with pytest.raises(m.McorrError):
            m.motion_correct_movies([torch.zeros(2, 64, 64)], 1.0)


def test_deformation_field_csv_round_trip_and_wire_format(tmp_path):
    """N4: CSV interchange identical to the reference's data_io.py (header, row order,
    float64 images of the float32 values; sorted-unique index axes on read)."""
    import torch_motion_correction_amd as m

    g = torch.Generator().manual_seed(4)
    field = torch.randn(2, 3, 2, 4, generator=g)
    p = tmp_path / "sub" / "field.csv"
    m.write_deformation_field_to_csv(field, p)
    lines = p.read_text().strip().split("\n")
    assert lines[0] == "t,h,w,y_shift,x_shift" and len(lines) == 1 + 3 * 2 * 4
    # the reference's own writer, element by element (data_io.py:39-62)
    t_, h_, w_, y_, x_ = lines[1 + (1 * 2 + 1) * 4 + 2].split(",")
    assert (int(t_), int(h_), int(w_)) == (1, 1, 2)
    assert float(y_) == field[0, 1, 1, 2].item() and float(x_) == field[1, 1, 1, 2].item()
    assert y_ == repr(field[0, 1, 1, 2].item())
    back = m.read_deformation_field_from_csv(p)
    assert back.dtype == torch.float32 and back.device.type == "cpu" and torch.equal(back, field)
    # non-contiguous index values: axes are the sorted sets of values (data_io.py:103-120)
    q = tmp_path / "gaps.csv"
    q.write_text("t,h,w,y_shift,x_shift\n5,0,7,1.5,-2.0\n2,0,3,0.25,4.0\n")
    gaps = m.read_deformation_field_from_csv(q)
    assert gaps.shape == (2, 2, 1, 2)
    assert gaps[0, 0, 0, 0] == 0.25 and gaps[1, 1, 0, 1] == -2.0 and gaps[0, 1, 0, 0] == 0.0
    with pytest.raises(ValueError):
        m.write_deformation_field_to_csv(torch.zeros(3, 2, 2), p)


@pytest.mark.parametrize("src", ["host_wave_fft.cpp", "host_wave_fft512.cpp", "host_wave_fft1024.cpp"])
def test_wave_fft_index_algebra_on_the_host(tmp_path, src):
    """csrc/mc_wave_fft.h is written __host__ __device__: the lane ownership, slab addressing,
    pruned butterflies and in-lane / lane-permute real-FFT unpack of both wave transforms
    (2048- and 512-point rows, 1024-point columns) are executed lane by lane on the CPU and compared with a
    double-precision DFT.  Needs clang++ (ext_vector_type); the ROCm one is used."""
    run_host_program(src, tmp_path, sanitize=False)


def test_every_name_the_reference_exports_is_exported_here():
    """src/torch_motion_correction/__init__.py:31-43 (__all__ of the reference)."""
    import torch_motion_correction_amd as mc

    reference_all = ["estimate_local_motion", "correct_motion", "correct_motion_two_grids", "correct_motion_fast",
                     "correct_motion_slow", "get_pixel_shifts", "evaluate_deformation_field",
                     "estimate_global_motion", "estimate_motion_cross_correlation_patches",
                     "write_deformation_field_to_csv", "read_deformation_field_from_csv"]
    for name in reference_all:
        assert name in mc.__all__ and callable(getattr(mc, name)), name
    import inspect

    sig = inspect.signature(mc.estimate_local_motion)
    assert list(sig.parameters) == ["image", "pixel_spacing", "patch_shape", "deformation_field_resolution",
                                    "initial_deformation_field", "device", "n_iterations", "b_factor",
                                    "frequency_range", "optimizer_type", "grid_type", "loss_type",
                                    "optimizer_kwargs", "return_trajectory", "trajectory_kwargs"]  # :28-44
    assert sig.parameters["n_iterations"].default == 100 and sig.parameters["loss_type"].default == "mse"
    assert list(inspect.signature(mc.correct_motion_two_grids).parameters) == [
        "image", "new_deformation_grid", "base_deformation_grid", "pixel_spacing", "grad", "device"]
    assert list(inspect.signature(mc.correct_motion_slow).parameters) == ["image", "deformation_grid", "grad", "device"]


def test_three_operation_division_is_the_correctly_rounded_quotient():
    """warp_common.h grid_chain divides by the invariant d = 0.5 n - 0.5 as q = c r; e = fma(-q, d, c);
    q' = fma(e, r, q).  Checked here against exact rational arithmetic (the reference divides)."""
    from fractions import Fraction
    import math

    def rn32(fr):
        if fr == 0:
            return np.float32(0)
        sgn = 1 if fr > 0 else -1
        fr = abs(fr)
        e = math.floor(math.log2(fr))
        while Fraction(2) ** e > fr:
            e -= 1
        while Fraction(2) ** (e + 1) <= fr:
            e += 1
        scaled = fr / Fraction(2) ** e * (1 << 23)
        fl = scaled.numerator // scaled.denominator
        rem = scaled - fl
        if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
            fl += 1
        return np.float32(sgn * float(fl) * 2.0 ** (e - 23))

    rng = np.random.default_rng(0)
    for n in (64, 959, 4092, 4096, 5760, 8184, 11520):
        d = np.float32(0.5) * np.float32(n) - np.float32(0.5)
        r = np.float32(1.0) / d
        a = (rng.random(300, dtype=np.float32) * np.float32(n + 40) - np.float32(20)).astype(np.float32)
        a[:100] = np.round(a[:100]) + rng.choice([0, 1e-4, -1e-4, 0.5], 100).astype(np.float32)
        for x in a:
            q = np.float32(x * r)
            e = rn32(Fraction(float(x)) - Fraction(float(q)) * Fraction(float(d)))
            q1 = rn32(Fraction(float(q)) + Fraction(float(e)) * Fraction(float(r)))
            assert q1 == rn32(Fraction(float(x)) / Fraction(float(d))), (n, x)


def test_row_chords_bracket_every_nonzero_mask_value():
    """plan.row_chords: the per-row clamp range K1 uses must contain every non-zero mask sample
    (a missed one would be replaced by a clamped neighbour) and is tight to 4-sample quads."""
    mask = tp.circle(40.0, (128, 160), smoothing_radius=20.0)
    ch = plan.row_chords(mask)
    assert ch.shape == (128, 2) and ch.dtype == torch.int32
    for y in range(128):
        nz = torch.nonzero(mask[y]).flatten()
        lo, hi = int(ch[y, 0]), int(ch[y, 1])
        assert lo % 4 == 0 and hi % 4 == 0 and 0 <= lo <= hi <= 156
        if len(nz):
            assert lo <= int(nz[0]) < lo + 4 and hi <= int(nz[-1]) < hi + 4
        else:
            assert lo == hi == 80
    # the reference's central statistics box lies inside the chords of the reference's mask
    h = w = 256
    m = tp.circle(min(h, w) / 4, (h, w), smoothing_radius=min(h, w) / 8)
    c = plan.row_chords(m)[int(0.25 * h):int(0.75 * h)]
    assert bool((c[:, 0] <= int(0.25 * w)).all()) and bool((c[:, 1] + 4 >= int(0.75 * w)).all())


def test_launches_refuse_a_device_that_is_not_current(monkeypatch):
    """libmcorr launches on the CURRENT HIP device; buffers elsewhere must fail loudly, not launch
    on the wrong GPU (the API enters _lib.device_scope(device) around every call)."""
    import torch
    from torch_motion_correction_amd import _lib

    monkeypatch.setattr(torch.cuda, "current_device", lambda: 1)
    with pytest.raises(_lib.McorrError, match="current device"):
        _lib.stream_ptr(torch.device("cuda:0"))
    with pytest.raises(_lib.McorrError, match="ROCm device"):
        _lib.stream_ptr(torch.device("cpu"))


def test_reference_frame_normalisation():
    from torch_motion_correction_amd import _lib

    assert _lib.normalize_frame_index(-1, 5) == 4 and _lib.normalize_frame_index(3, 5) == 3
    assert _lib.normalize_frame_index(-5, 5) == 0
    for bad in (5, -6, 100):
        with pytest.raises(IndexError):
            _lib.normalize_frame_index(bad, 5)
    with pytest.raises(TypeError):
        _lib.normalize_frame_index(1.5, 5)


def test_mask_schedule_with_a_negative_reference_key():
    """-1 and t-1 are two memo entries of the reference's LazyPatchGrid (the key is the raw int):
    no frame is skipped and the reference entry collects one mask factor per processed frame."""
    ref_expo, cur_expo, processed, ref_read = lattice.mask_schedule(5, "middle_frame", -1, with_ref_reads=True)
    assert processed == [0, 1, 2, 3, 4]
    assert ref_read.tolist() == [0, 1, 2, 3, 4] and cur_expo.tolist() == [0, 0, 0, 0, 0]
    ref_expo, cur_expo, processed, ref_read = lattice.mask_schedule(5, "middle_frame", 4, with_ref_reads=True)
    assert processed == [0, 1, 2, 3] and ref_read.tolist() == [0, 1, 2, 3, -1]


class _FakeResult:
    def __init__(self, field, total):
        self.field, self.total = field, total


class _FakePipeline:
    """CPU stand-in with MoviePipeline's iterate() contract: the 'field' of a movie is its
    per-frame mean (so the gathered table can be checked exactly), the 'sum' its frame sum."""

    def iterate(self, movies):
        for m in movies:
            f = torch.stack([m.mean(dim=(1, 2)), -m.mean(dim=(1, 2))])[:, :, None, None]
            yield _FakeResult(f, m.sum(0))


def _sharded_rank_main(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        loaded = []

        def load(i):
            loaded.append(i)
            return torch.full((3, 4, 5), float(i)) + torch.arange(3.0)[:, None, None]

        fields, sums = multi_gpu.motion_correct_movies_sharded(
            list(range(7)), rank, world, 1.0, load=load, pipeline_factory=_FakePipeline)
        q.put((rank, loaded, {k: v.tolist() for k, v in fields.items()}, sorted(sums)))
    finally:
        dist.destroy_process_group()


def test_sharded_driver_two_ranks_gloo():
    """motion_correct_movies_sharded: every rank touches only its round-robin shard, the fields of
    ALL movies come back on every rank, the sums stay with their rank (7 movies over 2 ranks)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_sharded_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (r0, l0, f0, s0), (r1, l1, f1, s1) = results
    assert l0 == [0, 2, 4, 6] and l1 == [1, 3, 5] and s0 == l0 and s1 == l1
    assert f0 == f1 and sorted(f0) == list(range(7))
    for i in range(7):
        assert f0[i][0] == [[[float(i)]], [[float(i) + 1]], [[float(i) + 2]]]


def test_sharded_driver_single_rank_needs_no_process_group():
    fields, sums = multi_gpu.motion_correct_movies_sharded(
        [torch.ones(2, 3, 3) * k for k in range(3)], 0, 1, 1.0, pipeline_factory=_FakePipeline)
    assert sorted(fields) == [0, 1, 2] and sorted(sums) == [0, 1, 2]
    assert float(sums[2].sum()) == 2 * 2 * 9
