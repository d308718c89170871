"""The kernels of the iterative estimators (csrc/local_motion.hip, csrc/xc_refine.hip, csrc/xc_refine_patches.hip)
through the C entry points, against the float64 definitions of tests/iteration_reference.py, whose docstring derives
every bound.  No element, bin, frame or patch is skipped: every output buffer is pre-filled with a sentinel that lies
outside every bound (an element that is not written fails its comparison) and sits between two guard regions that must
come back bit-unchanged.

Cases (shared with tests/test_iteration_reference_host.py):

  loss kernels, (npatch, t, nkx, nky), tiles of 1024 bins:
    (1, 2, 1, 1)      one bin, smallest t            (2, 5, 5, 9)      45 bins, the regime of the older tests (control)
    (3, 3, 16, 64)    exactly one tile               (2, 4, 25, 41)    a second tile that holds one bin
    (2, 7, 33, 65)    three tiles, the last with 97 bins: lanes break in the middle of a sweep
    (1, 3, 1100, 1), (1, 3, 1, 1100)   degenerate index splits
    (1, 130, 3, 7)    2 t > 256: the second sweep of the LDS shift load, 33 rounds of the wave-per-frame loop
    (1, 512, 7, 10)   LDS tables full
   each with hx = NULL / Hermitian 1, 2, .., 2, 1 / arbitrary, and shifts zero / half-integers / random / (-200.25, 180.5)
   / the aligned stack, where the sums cancel and only an absolute bound says anything; ab random of both signs.
  mc_xc_aligned_refs (t, nkx, nky, under): one frame (REF exactly 0), one workgroup exactly, one bin in a second
   workgroup, nky = 1, the unroll remainder with t > 64, t = 512; the patch form with 5 patches, the ranges (0, 5),
   (2, 2), (4, 1), whole-pixel offsets (s - o cancelling in two patches); npatch = 1 with zero offsets is bit-equal to
   the plain kernel.
  update kernels: t in {2, 6, 64, 65, 130, 512}, ref in {0, t // 2, t - 1}, (96, 120) and (9, 11); the frame kinds of
   iteration_reference.update_case; the patch form on the three ranges with everything outside bit-unchanged; one
   patch is bit-equal to the plain kernel.
  LocalMotionProblem on a (3, 384, 384) stack with 256-px patches: ntiles > 1, sums and ncc_grad_sums against the
   float64 definitions applied to its own spectra.

Worst error / bound: this file prints RATIO lines; DESIGN.md section 6 records them, from a complete run on an MI355X,
next to the fp32 CPU stand-in's ratios of the host test.
"""

import ctypes as C

import numpy as np
import pytest
import torch

import iteration_reference as ir
from kernel_harness import ratios_fixture, worse

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 32


def _api():
    from torch_motion_correction_amd import _lib
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    return _lib.load(), check, ptr, stream_ptr


def _ids(c):
    return "x".join(map(str, c)) if isinstance(c, tuple) else str(c)


ratios = ratios_fixture()


class _Guarded:
    """A device buffer between two guard regions.  `init`: a numpy array (an in / out argument), or a shape (an output,
    pre-filled with the sentinel)."""

    def __init__(self, init, dev, dtype=torch.float32):
        shape = init.shape if isinstance(init, np.ndarray) else tuple(init)
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * GUARD,), ir.SENTINEL, dtype=dtype, device=dev)
        self.t = self.whole[GUARD:GUARD + n].view(shape)
        if isinstance(init, np.ndarray):
            self.t.copy_(torch.from_numpy(init))
        self.n = n

    def read(self, what):
        w = self.whole.cpu().numpy()
        assert (w[:GUARD] == F32(ir.SENTINEL)).all() and (w[GUARD + self.n:] == F32(ir.SENTINEL)).all(), \
            f"{what}: wrote outside its buffer"
        return w[GUARD:GUARD + self.n].reshape(tuple(self.t.shape)).copy()


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ mc_local_loss_sums, mc_local_ncc_grad


def _loss_launch(mode, Pd, sd, fyd, fxd, hd, abd, case, dev, what):
    lib, check, ptr, stream_ptr = _api()
    npatch, t, nkx, nky = case
    out = _Guarded((npatch, ir.ntiles(nkx, nky), t, 6 if mode == 0 else 2), dev)
    if mode == 0:
        rc = lib.mc_local_loss_sums(ptr(Pd), ptr(sd), ptr(fyd), ptr(fxd), ptr(hd), npatch, t, nkx, nky, ptr(out.t), stream_ptr(dev))
    else:
        rc = lib.mc_local_ncc_grad(ptr(Pd), ptr(sd), ptr(fyd), ptr(fxd), ptr(hd), ptr(abd), npatch, t, nkx, nky, ptr(out.t),
                                   stream_ptr(dev))
    check(rc, what)
    torch.cuda.synchronize()
    return out.read(what)


@pytest.mark.parametrize("case", ir.LOSS_CASES, ids=_ids)
def test_loss_kernels_match_float64(dev, ratios, case):
    lib, check, _, _ = _api()
    npatch, t, nkx, nky = case
    nt = C.c_int(0)
    check(lib.mc_local_loss_tiles(nkx, nky, C.byref(nt)), "mc_local_loss_tiles")
    assert nt.value == ir.ntiles(nkx, nky)
    worst = [0.0, 0.0]
    for sf in ir.SHIFT_FORMS:
        c = ir.loss_case(case, sf)
        Pd, sd, fyd, fxd, abd = (_dev(c[k], dev) for k in ("P", "shifts", "fy", "fx", "ab"))  # named: they outlive the launches
        for hf in ir.HX_FORMS:
            hx = ir.make_hx(hf, nkx)
            hd = _dev(hx, dev)
            what = f"{_ids(case)} {sf} hx={hf}"
            ref, bound = ir.loss_tiles64(c["P"], c["shifts"], c["fy"], c["fx"], hx)
            got = _loss_launch(0, Pd, sd, fyd, fxd, hd, None, case, dev, f"mc_local_loss_sums {what}")
            worst[0] = max(worst[0], ir.assert_within(got, ref, bound, f"mc_local_loss_sums {what}"))
            ref, bound = ir.ncc_grad_tiles64(c["P"], c["shifts"], c["fy"], c["fx"], hx, c["ab"])
            got = _loss_launch(1, Pd, sd, fyd, fxd, hd, abd, case, dev, f"mc_local_ncc_grad {what}")
            worst[1] = max(worst[1], ir.assert_within(got, ref, bound, f"mc_local_ncc_grad {what}"))
    print(f"RATIO loss kernels {_ids(case)}: sums {worst[0]:.3f} ncc grad {worst[1]:.3f}")
    worse(ratios, "mc_local_loss_sums", worst[0])
    worse(ratios, "mc_local_ncc_grad", worst[1])


def test_local_motion_problem_runs_more_than_one_tile(dev, ratios):
    """The real LocalMotionProblem at a shape with ntiles > 1: its sums / ncc_grad_sums (the tiles added in float64 by
    the Python layer) against the float64 definitions applied to its own spectra, the bounds of the tiles added."""
    from torch_motion_correction_amd import local_motion

    g = torch.Generator().manual_seed(5)
    stack = torch.randn(3, 384, 384, generator=g)
    prob = local_motion.LocalMotionProblem(stack.to(dev), 1.0, (256, 256), (3, 2, 2), "catmull_rom")
    assert prob.ntiles > 1 and prob.ntiles == ir.ntiles(prob.nkx, prob.nky)
    assert prob.nkx != prob.nky and 1024 < prob.nkx * prob.nky
    npatch, t = prob.npatch, prob.t
    P = prob.spectra.cpu().numpy().reshape(npatch, t, prob.nkx, prob.nky, 2)
    fy, fx, hx = prob.fy.cpu().numpy(), prob.fx.cpu().numpy(), prob.hx.cpu().numpy()
    assert (fy < 0).any()
    r = np.random.default_rng(9)
    shifts = r.uniform(-3, 3, (npatch, t, 2)).astype(F32)
    ab = r.normal(0, 1, (npatch, t, 2)).astype(F32)
    sd, abd = torch.from_numpy(shifts).to(dev), torch.from_numpy(ab).to(dev)
    for loss_type, hermitian in (("mse", False), ("cc", True), ("ncc", True)):
        got = prob.sums(sd, hermitian)
        torch.cuda.synchronize()
        ref, bound = ir.loss_tiles64(P, shifts, fy, fx, hx if hermitian else None)
        rr = ir.assert_within(got.cpu().numpy(), ref.sum(axis=1), bound.sum(axis=1), f"LocalMotionProblem.sums {loss_type}")
        worse(ratios, "LocalMotionProblem.sums", rr)
        print(f"RATIO LocalMotionProblem.sums {loss_type} ({prob.nkx} x {prob.nky} bins, {prob.ntiles} tiles): {rr:.3f}")
    got = prob.ncc_grad_sums(sd, abd)
    torch.cuda.synchronize()
    ref, bound = ir.ncc_grad_tiles64(P, shifts, fy, fx, hx, ab)
    rr = ir.assert_within(got.cpu().numpy(), ref.sum(axis=1), bound.sum(axis=1), "LocalMotionProblem.ncc_grad_sums")
    worse(ratios, "LocalMotionProblem.ncc_grad_sums", rr)
    print(f"RATIO LocalMotionProblem.ncc_grad_sums: {rr:.3f}")


# ------------------------------------------------------------------ mc_xc_aligned_refs and its patch form


def _refs_plain(Sd, sd, fyd, fxd, case, dev):
    lib, check, ptr, stream_ptr = _api()
    t, nkx, nky, under = case
    G, REF = _Guarded((t, nkx, nky, 2), dev), _Guarded((t, nkx, nky, 2), dev)
    check(lib.mc_xc_aligned_refs(ptr(Sd), ptr(sd), ptr(fyd), ptr(fxd), ptr(G.t), ptr(REF.t), t, nkx, nky, under, stream_ptr(dev)),
          "mc_xc_aligned_refs")
    torch.cuda.synchronize()
    return G.read("mc_xc_aligned_refs G"), REF.read("mc_xc_aligned_refs REF")


def _refs_patches(Sd, sd, od, fyd, fxd, case, npatch, q0, nq, dev):
    lib, check, ptr, stream_ptr = _api()
    t, nkx, nky, under = case
    G, REF = _Guarded((t, nq, nkx, nky, 2), dev), _Guarded((t, nq, nkx, nky, 2), dev)
    check(lib.mc_xc_aligned_refs_patches(ptr(Sd), ptr(sd), ptr(od), ptr(fyd), ptr(fxd), ptr(G.t), ptr(REF.t), t, npatch, q0, nq,
                                         nkx, nky, under, stream_ptr(dev)), "mc_xc_aligned_refs_patches")
    torch.cuda.synchronize()
    return G.read("mc_xc_aligned_refs_patches G"), REF.read("mc_xc_aligned_refs_patches REF")


@pytest.mark.parametrize("case", ir.ALIGNED_CASES, ids=_ids)
def test_aligned_refs_match_float64(dev, ratios, case):
    t, nkx, nky, under = case
    c = ir.aligned_case(case)
    Sd, sd, fyd, fxd = (_dev(c[k], dev) for k in ("S", "shifts", "fy", "fx"))
    G, REF = _refs_plain(Sd, sd, fyd, fxd, case, dev)
    rg, rr = ir.check_aligned(G, REF, ir.aligned_refs64(c["S"], c["shifts"], c["fy"], c["fx"], under, True),
                              f"mc_xc_aligned_refs {_ids(case)}")
    # "statement for statement": one patch with zero offsets is the plain kernel, bit for bit
    zd = torch.zeros((t, 1, 2), dtype=torch.float32, device=dev)
    G1, REF1 = _refs_patches(Sd, sd, zd, fyd, fxd, case, 1, 0, 1, dev)
    assert np.array_equal(G1[:, 0].view(np.uint32), G.view(np.uint32)), "the patch form with one patch is not bit-equal (G)"
    assert np.array_equal(REF1[:, 0].view(np.uint32), REF.view(np.uint32)), "the patch form with one patch is not bit-equal (REF)"
    p = ir.aligned_patch_case(case)
    pSd, psd, pod = (_dev(p[k], dev) for k in ("S", "shifts", "offsets"))
    pg = pr = 0.0
    for q0, nq in ir.PATCH_RANGES:
        Gp, REFp = _refs_patches(pSd, psd, pod, fyd, fxd, case, ir.NPATCH, q0, nq, dev)
        ref4 = ir.aligned_refs_patches64(p["S"], p["shifts"], p["offsets"], p["fy"], p["fx"], under, q0, nq, True)
        a, b = ir.check_aligned(Gp, REFp, ref4, f"mc_xc_aligned_refs_patches {_ids(case)} range {(q0, nq)}")
        pg, pr = max(pg, a), max(pr, b)
    print(f"RATIO aligned refs {_ids(case)}: G' {rg:.3f} REF {rr:.3f}; patches G' {pg:.3f} REF {pr:.3f}")
    worse(ratios, "mc_xc_aligned_refs G'", rg)
    worse(ratios, "mc_xc_aligned_refs REF", rr)
    worse(ratios, "mc_xc_aligned_refs_patches G'", pg)
    worse(ratios, "mc_xc_aligned_refs_patches REF", pr)


# ------------------------------------------------------------------ mc_xc_refine_update and its patch form


def _update_plain(pd, nd, shifts, ref, t, H, W, under, dev):
    lib, check, ptr, stream_ptr = _api()
    s, m = _Guarded(shifts, dev), _Guarded((1,), dev)
    check(lib.mc_xc_refine_update(ptr(pd), ptr(nd), ptr(s.t), ref, t, H, W, under, ptr(m.t), stream_ptr(dev)),
          "mc_xc_refine_update")
    torch.cuda.synchronize()
    return s.read("mc_xc_refine_update shifts"), m.read("mc_xc_refine_update max_r")


def _update_patches(pd, nd, shifts, max_r, ref, t, npatch, q0, nq, H, W, under, dev):
    lib, check, ptr, stream_ptr = _api()
    s, m = _Guarded(shifts, dev), _Guarded(max_r, dev)
    check(lib.mc_xc_refine_update_patches(ptr(pd), ptr(nd), ptr(s.t), ref, t, npatch, q0, nq, H, W, under, ptr(m.t),
                                          stream_ptr(dev)), "mc_xc_refine_update_patches")
    torch.cuda.synchronize()
    return s.read("mc_xc_refine_update_patches shifts"), m.read("mc_xc_refine_update_patches max_r")


@pytest.mark.parametrize("t", ir.UPDATE_T)
def test_update_kernels_match_float64(dev, ratios, t):
    w = dict(s=0.0, m=0.0, ps=0.0, pm=0.0)
    for (H, W), under in ir.UPDATE_SHAPES:
        for v in range(3):
            c = ir.update_case(t, v, (H, W), under)
            what = f"t={t} ref={c['ref']} {(H, W)}"
            pd, nd = _dev(c["peaks"], dev), _dev(c["nb"], dev)
            s, m = _update_plain(pd, nd, c["shifts"], c["ref"], t, H, W, under, dev)
            ref4 = ir.refine_update64(c["peaks"], c["nb"], c["shifts"], c["ref"], H, W, under, bounds=True)
            a, b = ir.check_update(s, m, ref4, c["ref"], f"mc_xc_refine_update {what}")
            w["s"], w["m"] = max(w["s"], a), max(w["m"], b)
            # one patch is the plain kernel, bit for bit
            s1, m1 = _update_patches(pd, nd, c["shifts"][:, None], np.full(1, ir.SENTINEL, dtype=F32), c["ref"], t, 1, 0, 1, H, W,
                                     under, dev)
            assert np.array_equal(s1[:, 0].view(np.uint32), s.view(np.uint32)), f"{what}: one patch is not bit-equal (shifts)"
            assert np.array_equal(m1.view(np.uint32), m.view(np.uint32)), f"{what}: one patch is not bit-equal (max_r)"
            for q0, nq in ir.PATCH_RANGES:
                p = ir.update_patch_case(t, v, (H, W), under, q0, nq)
                ppd, pnd = _dev(p["peaks"], dev), _dev(p["nb"], dev)
                sp, mp = _update_patches(ppd, pnd, p["shifts"], p["max_r"], p["ref"], t, ir.NPATCH, q0, nq, H, W, under, dev)
                ref4 = ir.refine_update_patches64(p["peaks"], p["nb"], p["shifts"], p["ref"], q0, nq, H, W, under, p["max_r"], True)
                a, b = ir.check_update_patches(sp, mp, p["shifts"], p["max_r"], ref4, p["ref"], q0, nq,
                                               f"mc_xc_refine_update_patches {what} range {(q0, nq)}")
                w["ps"], w["pm"] = max(w["ps"], a), max(w["pm"], b)
    print(f"RATIO update kernels t={t}: shifts {w['s']:.3f} max_r {w['m']:.3f}; patches shifts {w['ps']:.3f} max_r {w['pm']:.3f}")
    worse(ratios, "mc_xc_refine_update shifts", w["s"])
    worse(ratios, "mc_xc_refine_update max_r", w["m"])
    worse(ratios, "mc_xc_refine_update_patches shifts", w["ps"])
    worse(ratios, "mc_xc_refine_update_patches max_r", w["pm"])
