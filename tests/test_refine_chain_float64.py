"""The iterative sub-pixel routes on the GPU -- refine_global_motion[_raw], refine_local_motion -- judged as a whole
chain by the derived float64 bound of tests/refine_chain_reference.py (its docstring derives every term; none is fitted
to a kernel's output): ITER iterations on both sides with convergence_threshold = 0, every frame, patch and axis of the
field within its own bound, the per-iteration max |r| within its bound, the reference frame's row exactly 0.  Each test
asserts which entry points ran (kernel_harness.calls): a route that fell back to another kernel does not count.
torch.empty hands out NaN (nan_empty), so a value a kernel leaves unwritten fails its comparison.

tests/test_refine_chain_host.py checks, without a GPU, the fitness conditions of every case, that an fp32 stand-in of
the chain lies inside the bound and that planted faults of the chain leave it."""

import numpy as np
import pytest
import torch

import refine_chain_reference as rc
import xc_reference as xr
from kernel_harness import calls, mc, nan_empty, switches  # noqa: F401

pytestmark = pytest.mark.gpu

ITER = rc.ITER
SEPARATE = ("mc_xc_cols_inverse", "mc_xc_rows_inverse_argmax", "mc_xc_peak_neighbourhood")
FUSED = ("mc_xc_correlate_argmax",)
CHIRP = ("mc_xcg_cols_inverse", "mc_xcg_rows_inverse", "mc_xcg_peak_neighbourhood")


def _px(field, ps):
    """(2, t, gh, gw) Angstrom on the device -> (t, npatch, 2) px, float64."""
    f = field.detach().cpu().double()
    return (f.permute(1, 2, 3, 0).reshape(f.shape[1], -1, 2) / ps).numpy()


def _report(c, got, hist, what):
    assert hist.device.type == "cpu" and tuple(hist.shape) == (ITER,)
    ratio, hr = rc.check(c, _px(got, c["case"].ps), hist.double().numpy(), what)
    print(f"RATIO refine chain {what}: field {ratio:.3f} of a bound of {c['bound'].max():.2e} px, history "
          f"{[round(x, 3) for x in hr]}")
    return ratio


def _search(c, fused):
    """The K3 / K4 / K6 entry points `_peaks` is meant to take for the case's plan."""
    kinds = xr.line_costs(xr.geometry(c["pa"]))["kinds"]
    if fused:
        assert kinds == {"rows": "native", "cols": "native"}
        return FUSED, SEPARATE + CHIRP
    cols = "mc_xc_cols_inverse" if kinds["cols"] == "native" else "mc_xcg_cols_inverse"
    rows = (("mc_xc_rows_inverse_argmax", "mc_xc_peak_neighbourhood") if kinds["rows"] == "native"
            else ("mc_xcg_rows_inverse", "mc_xcg_peak_neighbourhood"))
    want = (cols,) + rows
    return want, tuple(n for n in FUSED + SEPARATE + CHIRP if n not in want)


def _frame(mc, dev, calls, name, fused=False, extra=(), absent=(), stats=None):
    c = rc.reference(name, stats)
    rc.fitness(c)
    case, inp = c["case"], c["inputs"]
    t = case.shape[0]
    field = None if c["field"] is None else c["field"].to(dev)
    keep = None if field is None else field.clone()
    kw = dict(deformation_field=field, reference_frame=case.ref, frequency_range=case.freq, max_iterations=ITER,
              convergence_threshold=0, return_history=True)
    calls.clear()
    if inp["gain"] is None:
        got, hist = mc.refine_global_motion(inp["movie"].to(dev), case.ps, **kw)
    else:
        got, hist = mc.refine_global_motion_raw(inp["movie"].to(dev), inp["gain"].to(dev), case.ps, **kw)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, t, 1, 1)
    assert field is None or torch.equal(field, keep)
    want, without = _search(c, fused)
    calls.ran("mc_xc_aligned_refs", "mc_xc_refine_update", *want, *extra,
              absent=without + absent + ("mc_xc_aligned_refs_patches", "mc_xc_refine_update_patches"))
    assert calls.count("mc_xc_aligned_refs") == ITER and calls.count("mc_xc_refine_update") == ITER
    return c, _report(c, got, hist, name)


@pytest.mark.parametrize("name", [c.name for c in rc.FRAME_CASES if c.shape[1] < 1024])
def test_whole_frames_separate_search(mc, dev, calls, nan_empty, name):
    c, _ = _frame(mc, dev, calls, name)
    chirp = name in ("3x100x120", "3x121x135")
    assert ("mc_xcg_cols_inverse" in calls.names) == chirp, "the chirp-z cases, and only they, take the chirp-z engine"
    if name == "3x256x256-caller":
        assert c["field"] is not None and c["start"][c["ref"]].any()  # a start whose reference row is not 0


@pytest.mark.parametrize("fused", [True, False])
def test_whole_frames_1024(mc, dev, calls, nan_empty, switches, fused):
    engine, _ = switches
    engine.FUSED_SEARCH = fused
    _frame(mc, dev, calls, "3x1024x1024", fused)


@pytest.mark.parametrize("kind", list(rc.RAW_KINDS))
def test_raw_whole_frames(mc, dev, calls, nan_empty, kind):
    """u8 / i16 counts with a gain of 1 +- 0.1 through the fused raw row pass, against the restatement on the float64
    conditioning with the statistics the kernels were given."""
    from torch_motion_correction_amd import engine

    name = f"3x1024x1024-{kind}"
    raw, gain = rc.raw_counts(rc.CASES[name])
    rm = engine.RawMovie(raw.to(dev), gain.to(dev))
    torch.cuda.synchronize()
    stats = (rm.sub.cpu().numpy(), float(rm.mean_rstd.cpu()[1]))
    _frame(mc, dev, calls, name, True, ("mc_xc_rows_forward_raw",), ("mc_condition_movie",), stats)


def _patches(mc, dev, calls, name, fused, k1, extra=(), absent=()):
    c = rc.reference(name)
    rc.fitness(c)
    case, inp = c["case"], c["inputs"]
    kw = dict(deformation_field=c["field"].to(dev), reference_frame=case.ref, frequency_range=case.freq,
              max_iterations=ITER, convergence_threshold=0, return_history=True)
    calls.clear()
    if inp["gain"] is None:
        got, _, hist = mc.refine_local_motion(inp["movie"].to(dev), case.ps, case.p, **kw)
    else:
        got, _, hist = mc.refine_local_motion_raw(inp["movie"].to(dev), inp["gain"].to(dev), case.ps, case.p, **kw)
    torch.cuda.synchronize()
    want, without = _search(c, fused)
    calls.ran("mc_xc_aligned_refs_patches", "mc_xc_refine_update_patches", k1, *want, *extra,
              absent=without + absent + ("mc_xc_aligned_refs", "mc_xc_refine_update"))
    return c, got, hist


# name -> (patches, fused search): the wave-per-row row pass (mc_xc_rows_forward_dual_t) needs a plan of at most 128
# columns, which no input within the 1e-4 px fitness limit has (refine_chain_reference, REACH); these 1024-px patches
# take the workgroup row pass and the fused search
PATCHES = {"4x200x240-p96": (9, False), "4x512x640-p256": (6, False), "3x1537x1537-p1024": (4, True), "3x300x320-p256-one": (1, False)}


@pytest.mark.parametrize("name", list(PATCHES))
def test_patches(mc, dev, calls, nan_empty, name):
    npatch, fused = PATCHES[name]
    chirp = name == "4x200x240-p96"
    c, got, hist = _patches(mc, dev, calls, name, fused, "mc_xcg_rows_forward" if chirp else "mc_xc_rows_forward",
                            absent=("mc_xc_rows_forward_dual_t",))
    assert ("mc_xcg_cols_inverse" in calls.names) == chirp
    assert c["want"].shape[1] == npatch
    assert calls.count("mc_xc_aligned_refs_patches") == ITER  # one chunk
    _report(c, got, hist, name)


@pytest.mark.parametrize("kind", list(rc.RAW_KINDS))
def test_raw_patches(mc, dev, calls, nan_empty, kind):
    """u8 / i16 counts with a gain of 1 +- 0.1 through refine_local_motion_raw at 256-px patches: the route conditions
    the movie (mc_condition_movie) and runs the fp32 patch route; judged against the restatement on the float64
    conditioning, the conditioning roundings added to rel_S."""
    name = f"4x512x640-p256-{kind}"
    c, got, hist = _patches(mc, dev, calls, name, False, "mc_xc_rows_forward", extra=("mc_condition_movie",),
                            absent=("mc_xc_rows_forward_dual_raw",))
    _report(c, got, hist, name)


def test_patch_chunks_give_the_same_bits(mc, dev, calls, nan_empty, switches):
    """A small WORKSPACE_BYTES: 8 patches in chunks of 3, 3 and 2; the field is bit-equal to the one-chunk field and
    inside the bound."""
    engine, _ = switches
    name = rc.CHUNKED.name
    c, whole, _ = _patches(mc, dev, calls, name, False, "mc_xc_rows_forward")
    assert calls.count("mc_xc_aligned_refs_patches") == ITER
    a = calls.args["mc_xc_aligned_refs_patches"][0]
    t, npatch, nkx, nky = a[7], a[8], a[11], a[12]
    assert npatch == 8
    engine.WORKSPACE_BYTES = 3 * t * nkx * nky * 8
    c, got, hist = _patches(mc, dev, calls, name, False, "mc_xc_rows_forward")
    spans = [(x[9], x[10]) for x in calls.args["mc_xc_aligned_refs_patches"]]
    assert spans == [(0, 3), (3, 3), (6, 2)] * ITER, spans
    assert [(x[6], x[7]) for x in calls.args["mc_xc_refine_update_patches"]] == spans
    assert torch.equal(got, whole)
    _report(c, got, hist, f"{name} in 3 chunks")
