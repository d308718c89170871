"""Spline and lattice evaluation, the rigid and the deformation-field warp, pixel shifts.  (Named in the plural: the
package namespace holds the function ``warp``.)"""

from __future__ import annotations

import ctypes as C

import torch

from .. import _lib, engine as E, spline
from .._lib import check, ptr, stream_ptr


# ------------------------------------------------------------------ a14/a16: spline lattice


def spline_lattice(field, ut, uy, ux, grid_type):
    """Evaluate the (c,nt,nh,nw) spline grid `field` on the tensor-product lattice
    ut x uy x ux (CPU float32 coordinate vectors in [0,1]) -> (c, NT, NY, NX)."""
    lib = _lib.load()
    dev = field.device
    c, nt, nh, nw = field.shape
    tabs = []
    for n, u in ((nt, ut), (nh, uy), (nw, ux)):
        u = u.detach().to(torch.float32).cpu().contiguous()

        def build(n=n, u=u):
            idx, wts = spline.axis_taps(n, u, grid_type)
            return idx.to(dev), wts.to(dev), int(u.numel())

        tabs.append(E._cached(("taps", str(dev), n, grid_type, u.numpy().tobytes()), build))
    out = torch.empty((c, tabs[0][2], tabs[1][2], tabs[2][2]), dtype=torch.float32, device=dev)
    f = field.contiguous()
    check(lib.mc_spline_lattice(ptr(f), c, nt, nh, nw, ptr(tabs[0][0]), ptr(tabs[0][1]), tabs[0][2],
                                ptr(tabs[1][0]), ptr(tabs[1][1]), tabs[1][2], ptr(tabs[2][0]),
                                ptr(tabs[2][1]), tabs[2][2], ptr(out), stream_ptr(dev)),
          "mc_spline_lattice")
    return out


def spline_points(field, tyx, grid_type):
    """Evaluate the (c,nt,nh,nw) spline grid at (n, 3) points (t, y, x in [0,1], CPU float32) ->
    (n, c) on the device: ONE launch (tap tables per point built on the host)."""
    lib = _lib.load()
    dev = field.device
    c, nt, nh, nw = field.shape
    pts = tyx.detach().to(torch.float32).cpu().reshape(-1, 3)
    n = int(pts.shape[0])
    out = torch.empty((n, c), dtype=torch.float32, device=dev)
    if n == 0:
        return out
    tabs = [spline.axis_taps(size, pts[:, a].contiguous(), grid_type) for a, size in enumerate((nt, nh, nw))]
    dt = [(i.to(dev), w.to(dev)) for i, w in tabs]
    f = field.contiguous()
    check(lib.mc_spline_points(ptr(f), c, nt, nh, nw, ptr(dt[0][0]), ptr(dt[0][1]), ptr(dt[1][0]), ptr(dt[1][1]),
                               ptr(dt[2][0]), ptr(dt[2][1]), n, ptr(out), stream_ptr(dev)), "mc_spline_points")
    return out


def frame_lattices(field, t, grid_type):
    """(t, 2, 10gh, 10gw) Angstrom lattices, one per frame time linspace(0,1,t)
    (correct_motion.py:57,67-72)."""
    _, _, gh, gw = field.shape
    lin = lambda n: E._cached(("linspace", n), lambda: torch.linspace(0, 1, steps=n))
    lat = spline_lattice(field, lin(t), lin(10 * gh), lin(10 * gw), grid_type)
    return lat.permute(1, 0, 2, 3).contiguous()


# ------------------------------------------------------------------ a15/a17/a18: warp


def rigid_shifts_px(lattices, pixel_spacing):
    """(t, 2) fp32 pixel shifts of the rigid warp from the (t, 2, GH, GW) Angstrom lattices of a (2, t, 1, 1)
    field: the lattice value over the pixel spacing, the correctly rounded fp32 quotient -- the rule of rigid_tail,
    of the general-field kernel and of the reference (a CPU tensor over a Python float).  The divisor is a device
    tensor: ATen divides a CUDA tensor by a Python scalar as a multiply by fp32(1 / ps), which is one ulp off for
    some shifts (ps = 0.83: -3 px becomes -3 - 2.4e-7, and pixel row 3 falls outside the frame).  No host
    synchronisation."""
    ps = torch.full((), float(pixel_spacing), dtype=torch.float32, device=lattices.device)
    return torch.div(lattices[:, :, 0, 0], ps).contiguous()


def _rigid_scratch(lib, t, h, w, dev):
    """The rigid warp's scratch buffer (weight tables of t frames of h x w)."""
    nbytes = C.c_int64(0)
    check(lib.mc_warp_rigid_scratch_bytes(t, h, w, C.byref(nbytes)), "mc_warp_rigid_scratch_bytes")
    return torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)


def _field_scratch(lib, t, h, w, GH, GW, dev):
    """The deformation-field warp's scratch buffer for (GH, GW) lattices."""
    nbytes = C.c_int64(0)
    check(lib.mc_warp_scratch_bytes(t, h, w, GH, GW, C.byref(nbytes)), "mc_warp_scratch_bytes")
    return torch.empty((nbytes.value + 3) // 4, dtype=torch.float32, device=dev)


def _sum_target(out_sum, want_sum, accumulate, h, w, dev):
    """Where a raw warp's frame sum goes: the caller's `out_sum` (with `accumulate` the kernel adds to what it
    holds), a new (h, w) buffer with `want_sum`, else None."""
    if accumulate and out_sum is None:
        raise ValueError("accumulate needs out_sum")
    if out_sum is not None:
        return out_sum
    return torch.empty((h, w), dtype=torch.float32, device=dev) if want_sum else None


def rigid_tables(img, lattices, pixel_spacing):
    """The per-frame weight tables of the rigid warp (rigid_base + rigid_weights: phase 1 of
    mc_warp_rigid_phase_t) enqueued on the CURRENT stream -> an opaque handle for
    ``warp(..., rigid=True, tables=handle)``.  The movie pipeline builds them on the estimator's
    stream, so that the warp stream carries nothing but the resampling launch."""
    lib = _lib.load()
    t, h, w = img.shape
    dev = img.device
    shifts_px = rigid_shifts_px(lattices, pixel_spacing)
    scratch = _rigid_scratch(lib, t, h, w, dev)
    # phase 1 never touches the frames (only their geometry matters): tagged fp32 so that fp16 stacks of
    # any row length get their tables here, whichever kernel resamples them later
    check(lib.mc_warp_rigid_phase_t(ptr(img), E.STORE_F32, t, h, w, ptr(shifts_px), ptr(scratch), None, None, 1,
                                    stream_ptr(dev)), "mc_warp_rigid_phase_t")
    return shifts_px, scratch


def rigid_tables_from_shifts(shifts, img_shape, pixel_spacing, grid_type):
    """The movie pipeline's tail in two launches (mc_rigid_tables_from_shifts): (t,2) px shifts of the global
    estimate -> ((2,t,1,1) Angstrom field, handle for ``warp(..., rigid=True, tables=handle)``); the same
    numbers as image_shifts_to_deformation_field + frame_lattices + rigid_tables, bit for bit."""
    lib = _lib.load()
    t, h, w = img_shape
    dev = shifts.device

    def build():
        lin = torch.linspace(0, 1, steps=t)
        it, wt = spline.axis_taps(t, lin, grid_type)
        _, w1 = spline.axis_taps(1, torch.linspace(0, 1, steps=10)[:1], grid_type)  # lattice point 0 of a 1-sample axis
        return it.to(dev), wt.to(dev), w1[0].contiguous().to(dev)

    idx_t, w_t, w1 = E._cached(("rigid_tail_taps", str(dev), t, grid_type), build)
    field = torch.empty((2, t), dtype=torch.float32, device=dev)
    shifts_px = torch.empty((t, 2), dtype=torch.float32, device=dev)
    scratch = _rigid_scratch(lib, t, h, w, dev)
    check(lib.mc_rigid_tables_from_shifts(ptr(shifts.contiguous()), float(pixel_spacing), ptr(idx_t), ptr(w_t), ptr(w1),
                                          ptr(w1), t, h, w, ptr(field), ptr(shifts_px), ptr(scratch), stream_ptr(dev)),
          "mc_rigid_tables_from_shifts")
    return field[:, :, None, None], (shifts_px, scratch)


def warp(img, lattices, pixel_spacing, want_frames=True, want_sum=False, rigid=False, tables=None):
    """Resample every frame through its lattice; returns (frames or None, sum or None).
    rigid=True: the lattices come from a (2,nt,1,1) field, i.e. one shift per frame ->
    the separable rigid kernel (`tables`: the handle of an earlier ``rigid_tables`` call for
    the same stack and lattices; `lattices` may then be None)."""
    lib = _lib.load()
    t, h, w = img.shape
    dev = img.device
    if rigid and img.dtype == torch.float16 and (w % 8 or img.data_ptr() % 16):
        img = img.float()  # fp16 rows that are not whole 8-sample units: widened once
    frames = torch.empty((t, h, w), dtype=torch.float32, device=dev) if want_frames else None
    total = torch.empty((h, w), dtype=torch.float32, device=dev) if want_sum else None  # the kernels store it
    if rigid:
        if tables is None and E.RIGID_KERNEL_HOOK is not None:
            tables = rigid_tables(img, lattices, pixel_spacing)
        if tables is None:
            shifts_px = rigid_shifts_px(lattices, pixel_spacing)
            scratch = _rigid_scratch(lib, t, h, w, dev)
            args = (ptr(img), E.storage_of(img), t, h, w, ptr(shifts_px), ptr(scratch), ptr(frames), ptr(total))
            check(lib.mc_warp_rigid_phase_t(*args, 0, stream_ptr(dev)), "mc_warp_rigid_phase_t")
            return frames, total
        shifts_px, scratch = tables
        args = (ptr(img), E.storage_of(img), t, h, w, ptr(shifts_px), ptr(scratch), ptr(frames), ptr(total))
        run = lambda: check(lib.mc_warp_rigid_phase_t(*args, 2, stream_ptr(dev)), "mc_warp_rigid_phase_t")
        if E.RIGID_KERNEL_HOOK is None:
            run()
        else:  # instrumentation: the hook brackets the resampling kernel alone (bench.py)
            E.RIGID_KERNEL_HOOK(run)
        return frames, total
    _, _, GH, GW = lattices.shape
    scratch = _field_scratch(lib, t, h, w, GH, GW, dev)
    rc = lib.mc_warp_frames_t(ptr(img), E.storage_of(img), t, h, w, ptr(lattices), GH, GW, float(pixel_spacing),
                              ptr(scratch), ptr(frames), ptr(total), stream_ptr(dev))
    if rc == -2 and img.dtype != torch.float32:
        # fp16 frames outside the LDS-staged kernel's shapes (row length not a multiple of 8, dense
        # lattice): widen once and take the fp32 kernels
        rc = lib.mc_warp_frames_t(ptr(img.float()), E.STORE_F32, t, h, w, ptr(lattices), GH, GW, float(pixel_spacing),
                                  ptr(scratch), ptr(frames), ptr(total), stream_ptr(dev))
    check(rc, "mc_warp_frames_t")
    return frames, total


def pixel_shifts(lattice, h, w, pixel_spacing):
    """(h,w,2) px shifts from one (2,GH,GW) Angstrom lattice (correct_motion.py:132-185)."""
    lib = _lib.load()
    dev = lattice.device
    _, GH, GW = lattice.shape
    scratch = _field_scratch(lib, 1, h, w, GH, GW, dev)
    out = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
    check(lib.mc_pixel_shifts(ptr(lattice.contiguous()), GH, GW, h, w, float(pixel_spacing),
                              ptr(scratch), ptr(out), stream_ptr(dev)), "mc_pixel_shifts")
    return out


def pixel_shifts_at(lattice, h, w, pixel_spacing, coords):
    """get_pixel_shifts at arbitrary (..., 2) yx pixel coordinates (the reference's `pixel_grid`
    argument, correct_motion.py:167-168) -> (..., 2) px."""
    lib = _lib.load()
    dev = lattice.device
    _, GH, GW = lattice.shape
    pts = coords.reshape(-1, 2).contiguous()
    out = torch.empty_like(pts)
    if pts.shape[0]:
        check(lib.mc_pixel_shifts_at(ptr(lattice.contiguous()), GH, GW, h, w, float(pixel_spacing), ptr(pts),
                                     pts.shape[0], ptr(out), stream_ptr(dev)), "mc_pixel_shifts_at")
    return out.reshape(coords.shape)
