"""The derived bound of the composed refinement iteration (tests/refine_chain_reference.py), without a GPU: the fitness
conditions of every case of tests/test_refine_chain_float64.py; an fp32 stand-in of the chain -- the restatement run in
np.float32 (its `dtype` parameter: fp32 ramps, numpy's fp32 FFT, fp32 parabolas and updates; the spectra from torch's fp32
FFT, as tests/test_xc_reference_host.py forms its fp32 spectra) -- inside the bound on the smallest cases, which
shows that honest fp32 arithmetic can meet it; and the same stand-in with one fault planted, which must leave it:

  own frame        the current frame included in its own reference (REF_f = A / t)
  sign             the residual applied with the opposite sign on the x axis
  reference row    the reference frame's row updated like any other instead of held at 0
  stale            the shifts of the frame after the reference frame taken from the previous iteration when G is formed
  window offset    the window offset o not subtracted for patch 0 (cases whose windows moved: o != 0)

Each fault is a parameter of the restatement (global_refine_reference.FAULTS); nothing here runs on a GPU."""

import numpy as np
import pytest
import torch

import refine_chain_reference as rc
import xc_reference as xr

import global_refine_reference as gr

F32 = torch.float32
FAULTS = gr.FAULTS


def _spectra32(c):
    """fp32 spectra (t, npatch, H, W // 2 + 1) complex64 of the case's windows, in fp32 throughout."""
    case = c["case"]
    x = c["inputs"]["movie"]
    assert case.store in ("f32", "f16")
    x = x.float()
    t, h, w = x.shape
    pa = c["pa"]
    H, W = int(pa[0]), int(pa[1])
    box = x[:, int(0.25 * h):int(0.75 * h), int(0.25 * w):int(0.75 * w)]
    mean, std = box.mean(), box.std()
    mask, filt, _ = xr.tables64(pa)
    g = xr.geometry(pa)
    full = np.zeros((H, W // 2 + 1))
    full[xr.kept_rows(g)[:, None], np.arange(g.nkx)[None, :]] = filt.T
    mask32, filt32 = torch.from_numpy(mask).to(F32), torch.from_numpy(full).to(F32)
    if case.kind == "frame":
        corners = [[(0, 0)] for _ in range(t)]
    else:
        import local_refine_reference as lr

        _, _, origin = lr.patch_lattice(case.shape, case.p)
        o = np.stack([p.o for p in c["patches"]], axis=1).astype(np.int64)
        corners = [[tuple(origin[q] + o[f, q]) for q in range(len(origin))] for f in range(t)]
    S = torch.empty((t, len(corners[0]), H, W // 2 + 1), dtype=torch.complex64)
    for f in range(t):
        for q, (y0, x0) in enumerate(corners[f]):
            S[f, q] = torch.fft.rfft2((x[f, y0:y0 + H, x0:x0 + W] - mean) / std * mask32) * filt32
    return S


def standin(c, fault=None):
    """The restatement itself run in np.float32 on fp32 spectra -> (shifts (t, npatch, 2), history).  `fault`: one of
    global_refine_reference.FAULTS, a parameter of the restatement ('window offset': in patch 0 only)."""
    S = _spectra32(c).numpy()
    t, npatch = S.shape[:2]
    start = c["start"].astype(np.float32)
    out, hist = np.zeros((t, npatch, 2), dtype=np.float32), np.zeros((npatch, rc.ITER))
    for q, p in enumerate(c["patches"]):
        flt = None if (fault == "window offset" and q != 0) else fault
        out[:, q], res, _ = p.iterate(start[:, q], rc.ITER, full=S[:, q], dtype=np.float32, fault=flt)
        hist[q] = [np.abs(r).max() for r in res]
    return out, hist.max(axis=0)


ALL = list(rc.CASES)


@pytest.mark.parametrize("name", ALL)
def test_every_case_meets_the_fitness_conditions(name):
    c = rc.reference(name)
    print("TABLE " + rc.table_row(c))
    rc.fitness(c)


def test_patches_do_not_couple():
    rc.assert_patches_do_not_couple("4x512x640-p256")


@pytest.mark.parametrize("name", rc.SMALL)
def test_fp32_standin_lies_inside_the_bound(name):
    c = rc.reference(name)
    s, hist = standin(c)
    ratio, hr = rc.check(c, s, hist, f"fp32 stand-in {name}")
    print(f"RATIO fp32 stand-in {name}: field {ratio:.3f} history {[round(x, 3) for x in hr]}")
    print("TABLE " + rc.table_row(c, ratio))


# whole frames have no window offset to forget: that fault is planted in the patch cases
PLANTS = [(n, f) for n in rc.SMALL for f in FAULTS if not (f == "window offset" and rc.CASES[n].kind == "frame")]


@pytest.mark.parametrize("name,fault", PLANTS)
def test_planted_faults_leave_the_bound(name, fault):
    c = rc.reference(name)
    if fault == "window offset":
        assert c["patches"][0].o.any(), f"{name}: the windows of patch 0 did not move"
    s, hist = standin(c, fault)
    with pytest.raises(AssertionError):
        rc.check(c, s, hist, f"{fault} {name}")
