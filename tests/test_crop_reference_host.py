"""Host checks of tests/crop_reference.py -- the float64 definition of Fourier cropping, the column pass restated,
the derived bounds and the case tables of tests/test_crop_kernels_float64.py -- without a GPU: the restated column
pass between float64 row transforms IS the definition; the fp32 CPU oracle lies INSIDE the derived bounds on every
table case with a noise-like error (max / rms <= MAX_OVER_RMS, which licenses the per-element cap); and the bounds
DISCRIMINATE: every planted defect, applied to the float64 restatement, exceeds them at the tables' own inputs.

The identities of the definition (decimation of band-limited frames, linearity, kept sum, the Nyquist row's side) stay
in tests/test_fourier_crop_host.py."""

import math

import numpy as np
import pytest
import torch

import crop_reference as cr
import hot_reference as hr

U, F32 = cr.U, np.float32
ORACLE = {}  # family -> worst (L2, per element) ratio of the fp32 CPU oracle, printed at the end


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(ORACLE):
        print(f"ORACLE {k}: L2 {ORACLE[k][0]:.3f} element {ORACLE[k][1]:.3f}")


def _note(family, l2, px):
    a, b = ORACLE.get(family, (0.0, 0.0))
    ORACLE[family] = (max(a, l2), max(b, px))


# ------------------------------------------------------------------ the restatement is the definition


@pytest.mark.parametrize("h,w", [(16, 24), (32, 20), (12, 8), (64, 40)])
def test_column_pass_between_float64_row_transforms_is_the_definition(h, w):
    x = torch.randn(3, h, w, generator=torch.Generator().manual_seed(h * w), dtype=torch.float64) + 1.5
    S = cr.rows_forward64(x.numpy())
    assert S.shape == (3, h, w // 2 + 1)
    S2 = cr.cols_crop64(S, h, w)
    assert S2.shape == (3, h // 2, w // 4 + 1) and S2.dtype == np.complex128
    got = cr.rows_inverse64(S2, w)
    # crop_scale is 1 / ((h/2)(w/2)) rounded to fp32: inexact at these sizes, so the exact scale is put back
    got = got / cr.crop_scale(h, w) / ((h // 2) * (w // 2))
    assert np.abs(got - cr.crop64(x).numpy()).max() <= 1e-13 * float(x.abs().max())
    # columns beyond w/4 are ignored, fp32 pairs are read as complex values
    pairs = np.stack((S.real, S.imag), axis=-1).astype(F32)
    wide = np.concatenate((pairs, np.full_like(pairs[:, :, :3], np.nan)), axis=2)
    assert np.array_equal(cr.cols_crop64(wide, h, w), cr.cols_crop64(pairs[:, :, : w // 4 + 1], h, w))


def test_scale_is_the_kernels_rounding():
    assert cr.crop_scale(512, 128) == 1.0 / (256 * 64)  # powers of two: exact
    for h, w in [(8184, 128), (512, 11520), (8184, 11520)]:
        exact = 1.0 / ((h // 2) * (w // 2))
        assert cr.crop_scale(h, w) != exact and abs(cr.crop_scale(h, w) - exact) <= U * exact
    assert cr.A_CROP == math.sqrt(4096 * 4096 / (2048 * 2048))


# ------------------------------------------------------------------ the tables hold what the GPU tests need


def test_tables_cover_the_required_sizes():
    cols = set(cr.COLS_CASES)
    assert len(cr.COLS_CASES) == len(cols) == 13
    for h in (512, 1024, 2048, 4096, 8184):
        assert (h, 128) in cols
    for w in (128, 256, 512, 1024, 2048, 4096, 8192, 11520):
        assert (512, w) in cols
    assert (8184, 1024) in cols and cr.COLS_JOBS == 2
    routes = set(cr.ROUTE_CASES)
    assert len(cr.ROUTE_CASES) == len(routes)
    for c in [(2, 512, 128), (2, 1024, 256), (2, 2048, 128), (2, 4096, 128), (1, 8184, 128), (1, 8184, 1024)]:
        assert c + (0,) in routes
    for w in (512, 1024, 2048, 4096, 8192, 11520):
        assert (1, 512, w, 0) in routes
    assert sum(1 for c in cr.ROUTE_CASES if c[3] == 1) == 1  # one input 1 float past a 16-byte boundary
    assert (8184, 11520) not in {c[1:3] for c in cr.ROUTE_CASES} | cols  # nothing at the workload's own size
    assert cr.DISCARDED == (2, 512, 256) and cr.CHUNKS == (5, 512, 256) and cr.FP16 == (2, 512, 128)
    assert cr.RAW_SHAPE == (3, 512, 1024)
    assert set(cr.RAW_CASES) == {(d, m) for d in ("uint8", "int16") for m in (True, False)}
    # the widest column reference: 512 x 2881 complex128
    assert max((w // 4 + 1, h) for h, w in cr.COLS_CASES) == (2881, 512)
    from torch_motion_correction_amd import engine

    for h, w in list(cols) + [c[1:3] for c in cr.ROUTE_CASES] + [cr.DISCARDED[1:], cr.CHUNKS[1:], cr.RAW_SHAPE[1:]]:
        assert engine.fourier_crop_supported(h, w), (h, w)


def test_pitches_of_the_column_cases():
    """What the issue's shape list relies on: pitch2 = 48 (no remap: fewer than 8 groups of 8 pairs) at W = 128, and
    a remap with a tail (a group count that is no multiple of 8) at pitch2 = 144, 272, 2064, 2896."""
    from torch_motion_correction_amd import _lib

    lib = _lib.load()
    p2 = {w: lib.mc_full_spectrum_pitch(w // 2) for w in cr.COLS_WIDTHS}
    assert p2[128] == 48 and [p2[w] for w in (512, 1024, 8192, 11520)] == [144, 272, 2064, 2896]
    for w, p in p2.items():
        assert p == ((w // 4 + 1) + 15) // 16 * 16 and p >= w // 4 + 2
        groups = (p // 2 + 7) // 8
        assert (groups >= 8) == (w >= 512) and (w < 512 or groups % 8 != 0)


# ------------------------------------------------------------------ the fp32 oracle inside the bounds


def _oracle_cols32(S, H, W):
    """cols_crop64's steps with torch.fft in complex64."""
    z = torch.from_numpy(S[:, :, : W // 4 + 1].copy())
    z = torch.complex(z[..., 0], z[..., 1])
    F = torch.fft.fft(z, dim=1)
    G = torch.cat((F[:, : H // 4], F[:, H - H // 4:]), dim=1)
    out = torch.fft.ifft(G, dim=1) * F32(H // 2) * F32(cr.crop_scale(H, W))
    assert out.dtype == torch.complex64
    return out.numpy()


def _oracle_frames32(x):
    """rfft2, the crop, irfft2 in fp32."""
    x = x.float()
    h, w = x.shape[-2:]
    F = torch.fft.rfft2(x)
    G = torch.cat((F[..., : h // 4, : w // 4 + 1], F[..., h - h // 4:, : w // 4 + 1]), dim=-2)
    out = torch.fft.irfft2(G, s=(h // 2, w // 2))
    assert out.dtype == torch.float32
    return out


# the planted defects, on the cropped spectrum G (jobs or frames, H2, W/4 + 1) with F the uncropped one; `q` = H/4


def _changed(G, index, value):
    g = G.copy()
    g[index] = value
    return g


def _defects_on_spectrum(F, G, q, H):
    c = G.shape[2] // 3
    row = (slice(None), q)
    return {
        "Nyquist row from ky = +H/4": _changed(G, row, F[:, q]),
        "Nyquist row averaged from both sides": _changed(G, row, 0.5 * (F[:, q] + F[:, H - q])),
        # the band -H/4 <= ky <= H/4, one row too many, folded onto H/2 rows: both ends land on row H/4
        "kept rows off by one, ky <= H/4": _changed(G, row, F[:, q] + F[:, H - q]),
        "scale 1 / (H W)": 0.25 * G,
        "one output column left at zero": _changed(G, (0, slice(None), c), 0),
        "one output column holding its neighbour's values": _changed(G, (0, slice(None), c), G[0, :, c + 1]),
        "the column Nyquist kx = W/4 dropped": _changed(G, (slice(None), slice(None), -1), 0),
    }


@pytest.mark.parametrize("case", cr.COLS_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_column_pass_oracle_inside_the_bound_and_defects_outside(case):
    """Per column of every table case: the complex64 evaluation within cols_bound (L2 and per bin) with a noise-like
    error; every defect beyond it.  The criterion the defects are held to is the L2 bound of the worst column (the
    per-bin cap is exceeded as well wherever the L2 bound is exceeded by more than CAP, reported, not required)."""
    H, W = case
    S = cr.cols_input(H, W)
    ref = cr.cols_crop64(S, H, W)
    l2, px, peak = cr.cols_ratios(_oracle_cols32(S, H, W), ref, S, H, W)
    print(f"cols {H}x{W}: fp32 oracle L2 {l2:.3f} bin {px:.3f} max/rms {peak:.2f}")
    assert l2 <= 1 and px <= 1 and peak <= cr.MAX_OVER_RMS
    _note(f"cols H={H}", l2, px)
    z = cr._as_complex(S)
    F = np.fft.fft(z[:, :, : W // 4 + 1], axis=1)
    G = cr.cropped_columns64(S, H, W)
    bad = {k: cr.columns_inverse64(g, H, W) for k, g in _defects_on_spectrum(F, G, H // 4, H).items()}
    bad["two jobs swapped"] = ref[::-1]
    assert len(bad) == 8
    for name, got in bad.items():
        d_l2, d_px, _ = cr.cols_ratios(got, ref, S, H, W)
        print(f"  {name}: L2 {d_l2:.3g} bin {d_px:.3g}")
        assert d_l2 > 1, f"{name} passes the L2 bound at {case}: {d_l2}"


def _frame_defects(x64, partner64):
    """crop64 of one frame with each defect planted -> {name: (h/2, w/2) float64}."""
    h, w = x64.shape
    F = torch.fft.rfft2(x64)[None, :, : w // 4 + 1].numpy()
    G = np.concatenate((F[:, : h // 4], F[:, h - h // 4:]), axis=1)
    out = {k: torch.fft.irfft2(torch.from_numpy(g[0]), s=(h // 2, w // 2))
           for k, g in _defects_on_spectrum(F, G, h // 4, h).items()}
    out["two jobs swapped"] = cr.crop64(partner64)
    assert len(out) == 8
    return out


def _assert_frame_case(x, ref, oracle, partner, family, what, extra=None):
    """Every frame: the oracle inside frame_bound, its error noise-like; every defect beyond the L2 bound."""
    h, w = x.shape[-2:]
    for f in range(x.shape[0]):
        xf = x[f].double()
        b = cr.frame_bound(h, w, float(torch.linalg.norm(xf)), float(torch.linalg.norm(ref[f])),
                           0.0 if extra is None else float(extra[f]))
        l2, px = cr.frame_ratios(oracle[f], ref[f], b)
        d = oracle[f].double() - ref[f]
        peak = float(d.abs().max() / torch.sqrt((d * d).mean()))
        print(f"{what} frame {f}: fp32 oracle L2 {l2:.3f} pixel {px:.3f} max/rms {peak:.2f}")
        assert l2 <= 1 and px <= 1 and peak <= cr.MAX_OVER_RMS
        _note(family, l2, px)
        if f > 0:
            continue  # the defects are planted in the first frame
        other = x[1].double() if x.shape[0] > 1 else partner
        for name, got in _frame_defects(xf, other).items():
            d_l2, d_px = cr.frame_ratios(got, ref[f], b)
            print(f"  {name}: L2 {d_l2:.3g} pixel {d_px:.3g}")
            assert d_l2 > 1, f"{name} passes the L2 bound at {what}: {d_l2}"


@pytest.mark.parametrize("case", cr.ROUTE_CASES, ids=cr.case_id)
def test_frames_oracle_inside_the_bound_and_defects_outside(case):
    """The criterion the defects are held to is the per-frame L2 bound (the per-pixel ratio is printed)."""
    t, h, w, _ = case
    x, ref = cr.frames_reference(t, h, w)
    partner = cr.case_frames(1, h, w, other=True)[0].double() if t == 1 else None
    _assert_frame_case(x, ref, _oracle_frames32(x), partner, f"routes W={w}", f"frames {case[:3]}")


def test_chunked_case_oracle_inside_the_bound_and_defects_outside():
    t, h, w = cr.CHUNKS
    x, ref = cr.frames_reference(t, h, w)
    _assert_frame_case(x, ref, _oracle_frames32(x), None, "chunks", f"chunks {cr.CHUNKS}")


def test_fp16_case_oracle_inside_the_bound_and_defects_outside():
    t, h, w = cr.FP16
    x = cr.case_frames(t, h, w).half().float()
    _assert_frame_case(x, cr.crop64(x), _oracle_frames32(x), None, "fp16", f"fp16 {cr.FP16}")


def test_discarded_band_case():
    """The input's kept band holds its own fp32 rounding only: ||crop64(x)|| <= A u ||x|| (every sample moved by at
    most u |x|, through the factor A), so frame_bound is its forward term up to (c_inv + 2 u) A u ||x||; the fp32
    oracle is inside the forward term alone, and a bound relative to the OUTPUT's norm would be missed by orders of
    magnitude -- the case the old range criterion could not express.  The defects act on the kept band and vanish
    with it; here the planted fault is a kernel-like one instead: a forward pass that rounds a single
    row's samples to 1 / 256 leaks into the kept band beyond the bound."""
    t, h, w = cr.DISCARDED
    x = cr.discarded_band(t, h, w, seed=h + w)
    F = torch.fft.rfft2(x.double())
    kept = torch.cat((F[:, : h // 4, : w // 4 + 1], F[:, h - h // 4:, : w // 4 + 1]), dim=1)
    assert float(kept.abs().max()) <= 1e-4 * float(F.abs().max())
    ref, oracle = cr.crop64(x), _oracle_frames32(x)
    for f in range(t):
        xn, rn = float(torch.linalg.norm(x[f].double())), float(torch.linalg.norm(ref[f]))
        assert rn <= cr.A_CROP * U * xn
        b = cr.frame_bound(h, w, xn, rn)
        assert b["l2"] - b["fwd"] <= 1e-6 * b["fwd"]
        err = float(torch.linalg.norm(oracle[f].double() - ref[f]))
        print(f"discarded band frame {f}: ||ref|| / ||x|| {rn / xn:.2e}; oracle error / forward term {err / b['fwd']:.3f}, "
              f"error / ||ref|| {err / rn:.2f}")
        assert err <= b["fwd"] and float((oracle[f].double() - ref[f]).abs().max()) <= b["cap"]
        _note("discarded band", err / b["fwd"], float((oracle[f].double() - ref[f]).abs().max()) / b["cap"])
        assert err > 1e-3 * rn  # relative to the output the honest error is not small
        coarse = x[f].clone()
        coarse[7] = (coarse[7] * 256).round() / 256
        assert cr.frame_ratios(cr.crop64(coarse), ref[f], b)[0] > 1


def _mu32(raw, gain, mean_zero):
    """The fp32 frame means the kernels use, formed here in float64 and rounded (their accuracy is pinned in
    tests/test_hot_kernels_float64.py); zeros without mean_zero."""
    x = hr.product64(np.asarray(raw), np.asarray(gain))
    return (x.mean(axis=(1, 2)) if mean_zero else np.zeros(x.shape[0])).astype(F32)


@pytest.mark.parametrize("dtype,mean_zero", cr.RAW_CASES, ids=[f"{d}-{'mean_zero' if m else 'as_is'}" for d, m in cr.RAW_CASES])
def test_raw_cases_oracle_inside_the_bound_and_defects_outside(dtype, mean_zero):
    raw, gain = cr.raw_case(dtype)
    mu = _mu32(raw, gain, mean_zero)
    v, ref, cond = cr.raw_reference(raw.numpy(), gain.numpy(), mu)
    c32 = raw.float() * gain - torch.from_numpy(mu)[:, None, None]
    _assert_frame_case(torch.from_numpy(v), ref, _oracle_frames32(c32), None, "raw", f"raw {dtype} mean_zero={mean_zero}",
                       extra=cond)


def test_raw_hot_case_has_no_undecided_pixel_and_its_oracle_is_inside_the_bound():
    """hot_case() asserts that no pixel is undecided.  The oracle follows the kernels' order: the fp32 spectrum of
    the unreplaced conditioned samples plus each entry's correction, added in the spectrum."""
    raw, gain, ref, x = cr.hot_case()
    t, h, w = x.shape
    assert (ref.counts > 20).all() and len(ref.keys) == int(ref.counts.sum())
    mu = ref.mean_after.astype(F32)
    want, c_norm, extra, hot, more = cr.hot_reference_frames(raw, gain, ref, x, mu)
    v32 = hr.product32(raw, gain)
    c32 = torch.from_numpy(v32 - mu[:, None, None])
    assert c32.dtype == torch.float32
    S = torch.fft.rfft(c32, dim=2)
    h32 = hr.hot64(v32.astype(np.float64), cr.RAW_HOT[1])
    assert np.array_equal(h32.keys, ref.keys)
    kx = torch.arange(w // 2 + 1)
    for key, r in zip(ref.keys.tolist(), h32.r.astype(F32).tolist()):
        f, y, xx = key // (h * w), (key // w) % h, key % w
        dA = F32(r) - v32[f, y, xx]
        ang = (-2.0 * math.pi) * (((xx * kx) % w).float() / w)  # the phase reduced in integers, as the kernel's
        S[f, y] += torch.complex(torch.cos(ang), torch.sin(ang)) * float(dA)
    F = torch.fft.fft(S, dim=1)
    G = torch.cat((F[:, : h // 4, : w // 4 + 1], F[:, h - h // 4:, : w // 4 + 1]), dim=1)
    oracle = torch.fft.irfft2(G, s=(h // 2, w // 2))
    assert oracle.dtype == torch.float32
    for f in range(t):
        b = cr.frame_bound(h, w, c_norm[f], float(torch.linalg.norm(want[f])), extra[f], more, hot[f])
        l2, px = cr.frame_ratios(oracle[f], want[f], b)
        print(f"raw hot frame {f}: fp32 oracle L2 {l2:.3f} pixel {px:.3f}")
        assert l2 <= 1 and px <= 1
        _note("raw hot", l2, px)
        # the list matters: without the corrections the frame is far outside
        plain = _oracle_frames32(c32[f])
        assert cr.frame_ratios(plain, want[f], b)[0] > 1
