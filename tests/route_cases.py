"""The table of route cases: every entry point of include/mcorr.h at the smallest shape that still takes its kernel.

A case is a `make(dev) -> {name: input}` and a `route(**inputs)`; together the cases claim every stream-taking entry
point of the header (tests/test_stream_order.py holds the claims against the header and says what `proves`, `after`
and `rel` mean there).  tests/test_stream_order.py runs each case behind a delayed producer on a side stream,
tests/test_input_contract.py on inputs that start off a 16-byte boundary, with its inputs watched for writes, and
twice in different cache states.  A plain module: no test lives here."""

import numpy as np
import torch

import xc_reference as xr
from kernel_harness import float_stack, gain, raw_movie

BAND, BF = xr.DEFAULT_BAND, xr.B_FACTOR

# Routes whose statistics are accumulated with double atomics (condition.hip, hot_pixels.hip, the K1 statistics
# variants): the sums differ in their last bits from run to run, so do the floating-point outputs.  Their float64
# tests (test_hot_kernels_float64.py, test_xc_kernels_float64.py's fused-statistics cases) bound each element by an
# error model against a float64 reference, which has no meaning between two runs of the same kernel; here a run is
# compared with another run, against poison (NaN, or a movie's complement): 1e-4 of the output's largest value is far
# above the last bits and far below poison.  It applies to the floating-point results of these routes only: every
# integer result (counts, the counter, sorted keys) is compared bit for bit, as every result of every other route.
ATOMIC_REL = 1e-4


def E():
    from torch_motion_correction_amd import engine

    return engine


def _hot_movie(t, h, w, seed):
    raw = raw_movie(t, h, w, torch.uint8, seed)
    for f in range(t):
        for k in range(5):
            raw[f, (7 * k + 3 * f + 5) % h, (11 * k + 5 * f + 9) % w] = 255  # texture in [10, 50): hot by far
    return raw


def _rigid_field(t, dev):
    g = torch.Generator().manual_seed(t)
    return ((torch.rand(2, t, 1, 1, generator=g) - 0.5) * 5.0).to(dev)


def _shifts(t, dev):
    g = torch.Generator().manual_seed(t + 17)
    return ((torch.rand(t, 2, generator=g) - 0.5) * 6.0).to(dev)


class Case:
    """make(dev) -> {name: input}; route(**inputs) -> tensors; `proves`: entry points proven by the gated run;
    `after`: entry points of EXEMPT this case runs (stream argument and result checked); `rel`: None for bit-equal."""

    def __init__(self, name, make, route, proves, after=(), rel=None):
        self.name, self.make, self.route, self.proves, self.after, self.rel = name, make, route, proves, after, rel


CASES = []


def case(name, proves, after=(), rel=None):
    def deco(fn):
        make, route = fn()
        CASES.append(Case(name, make, route, tuple(proves), tuple(after), rel))
        return fn

    return deco


@case("global 512 fused statistics", ["mc_xc_provisional_mean_t", "mc_xc_rows_forward_stats_t",
                                      "mc_xc_cols_forward_fix", "mc_xc_cols_inverse", "mc_xc_rows_inverse_argmax"])
def _():
    return (lambda dev: dict(img=float_stack(3, 512, 512).to(dev)),
            lambda img: E().global_shifts(img, 1, 1.0, BF, BAND))  # whole-pixel arg-max: bit-equal


@case("global 1024 near-window search", ["mc_xc_correlate_argmax"])
def _():
    return (lambda dev: dict(img=float_stack(2, 1024, 1024).to(dev)),
            lambda img: E().global_shifts(img, 0, 1.0, BF, BAND))


@case("refined 512", ["mc_xc_aligned_refs", "mc_xc_peak_neighbourhood", "mc_xc_refine_update"], rel=ATOMIC_REL)
def _():
    return (lambda dev: dict(img=float_stack(3, 512, 512).to(dev)),
            lambda img: E().global_shifts_refined(img, 1, 1.0, BF, BAND, max_iterations=2, threshold=0.0)[0])


@case("refined chirp-z 96 x 160", ["mc_central_box_stats_t", "mc_xcg_rows_forward", "mc_xcg_cols_forward",
                                   "mc_xcg_cols_inverse", "mc_xcg_rows_inverse", "mc_xcg_peak_neighbourhood"],
      rel=ATOMIC_REL)
def _():
    return (lambda dev: dict(img=float_stack(3, 96, 160).to(dev)),
            lambda img: E().global_shifts_refined(img, 1, 1.0, BF, BAND, max_iterations=2, threshold=0.0)[0])


@case("fourier shift pruned 128 x 64", ["mc_xc_rows_forward", "mc_xc_cols_forward", "mc_fourier_shift_cols_inverse",
                                        "mc_xc_rows_inverse_store"])
def _():
    return (lambda dev: dict(img=float_stack(2, 128, 64).to(dev), shifts=_shifts(2, dev)),
            lambda img, shifts: E().fourier_shift(img, shifts))


@case("dose sum pruned 128 x 64", ["mc_dose_accumulate"])
def _():
    return (lambda dev: dict(img=float_stack(3, 128, 64).to(dev)),
            lambda img: E().dose_weighted_sum(img, 1.0, 1.2))


def _polyphase(fn):
    def run(**kw):
        eng = E()
        old, eng.POLYPHASE_FOURIER_SHIFT = eng.POLYPHASE_FOURIER_SHIFT, True
        try:
            return fn(eng, **kw)
        finally:
            eng.POLYPHASE_FOURIER_SHIFT = old

    return run


@case("polyphase 128 x 128", ["mc_polyphase_fourier_shift", "mc_polyphase_dose_accumulate"])
def _():
    return (lambda dev: dict(img=float_stack(2, 128, 128).to(dev), shifts=_shifts(2, dev)),
            _polyphase(lambda eng, img, shifts: (eng.fourier_shift(img, shifts), eng.dose_weighted_sum(img, 1.0, 1.2))))


@case("fourier shift row-major 256 x 64", ["mc_full_rows_forward", "mc_full_cols_shift", "mc_full_rows_inverse"])
def _():
    return (lambda dev: dict(img=float_stack(2, 256, 64).to(dev), shifts=_shifts(2, dev)),
            lambda img, shifts: E().fourier_shift(img, shifts))


@case("shift sums 256 x 64", ["mc_full_cols_shift_sum"])
def _():
    return (lambda dev: dict(img=float_stack(3, 256, 64).to(dev), shifts=_shifts(3, dev)),
            lambda img, shifts: E().fast_shift_sums(img, shifts, 1.0, 1.2, want_plain=True))


@case("shift sums column-major 4096 x 64", ["mc_full_transpose", "mc_full_cols_shift_sum_cm"])
def _():
    return (lambda dev: dict(img=float_stack(2, 4096, 64).to(dev), shifts=_shifts(2, dev)),
            lambda img, shifts: E().fast_shift_sums(img, shifts, 1.0, 1.2, want_plain=True))


@case("fourier crop 512 x 128", ["mc_full_cols_crop", "mc_full_cols_crop_to"])
def _():
    return (lambda dev: dict(img=float_stack(2, 512, 128).to(dev)),
            lambda img: (E().fourier_crop(img), E().fourier_crop_to(img, (384, 64))))


def _raw(t, h, w, hot, dev, dtype=torch.uint8):
    """A RawMovie built on the default stream: an input of a case, its tensors poisoned and restored like any other."""
    raw = _hot_movie(t, h, w, 3) if hot else raw_movie(t, h, w, dtype, 3)
    rm = E().RawMovie(raw.to(dev), gain(h, w).to(dev), hot_pixel_threshold=10.0 if hot else None)
    torch.cuda.synchronize()
    assert not hot or rm.n_hot >= 3  # (the detection rule keeps the strongest outliers)
    return rm


@case("raw shift sums 256 x 64", ["mc_full_rows_forward_raw"])
def _():
    return (lambda dev: dict(rm=_raw(3, 256, 64, False, dev), shifts=_shifts(3, dev)),
            lambda rm, shifts: E().fast_shift_sums(rm, shifts))


@case("raw shift sums with hot pixels", ["mc_full_rows_hot_correct"])
def _():
    return (lambda dev: dict(rm=_raw(3, 256, 64, True, dev), shifts=_shifts(3, dev)),
            lambda rm, shifts: E().fast_shift_sums(rm, shifts))


@case("raw movie statistics", ["mc_raw_movie_stats"], rel=ATOMIC_REL)
def _():
    def route(raw, g):
        rm = E().RawMovie(raw, g)
        return rm.mu, rm.sub, rm.mean_rstd

    return (lambda dev: dict(raw=raw_movie(3, 256, 64, torch.int16, 5).to(dev), g=gain(256, 64).to(dev)), route)


@case("raw hot-pixel list", ["mc_raw_hot_detect", "mc_raw_hot_finalize"], rel=ATOMIC_REL)
def _():
    """RawMovie.__init__ with a threshold reads the list's length back between the two entry points; here the length
    is an input (known from the default-stream run), so both are enqueued behind the gate."""
    def make(dev):
        raw = _hot_movie(3, 256, 64, 3).to(dev)
        g = gain(256, 64).to(dev)
        return dict(raw=raw, g=g, n=E().RawMovie(raw, g, hot_pixel_threshold=10.0).n_hot)

    def route(raw, g, n):
        from torch_motion_correction_amd import _lib
        from torch_motion_correction_amd._lib import check, ptr, stream_ptr

        lib, dev = _lib.load(), raw.device
        t, h, w = raw.shape
        hl, hu, wl, wu = int(0.25 * h), int(0.75 * h), int(0.25 * w), int(0.75 * w)
        cap = E().hot_list_capacity(t, h, w)
        stats, hstats = (torch.empty((t, 3), dtype=torch.float64, device=dev) for _ in range(2))
        mu, sub = torch.empty(t, dtype=torch.float32, device=dev), torch.empty(t, dtype=torch.float32, device=dev)
        mean_rstd = torch.empty(2, dtype=torch.float32, device=dev)
        keys = torch.empty(cap, dtype=torch.int64, device=dev)
        rv = torch.empty((cap, 2), dtype=torch.float32, device=dev)
        counter = torch.empty(1, dtype=torch.int64, device=dev)
        counts = torch.empty(t, dtype=torch.int32, device=dev)
        st = stream_ptr(dev)
        check(lib.mc_raw_hot_detect(ptr(raw), 0, ptr(g), t, h, w, hl, hu, wl, wu, 10.0, ptr(stats), ptr(hstats),
                                    ptr(keys), ptr(rv), cap, ptr(counter), ptr(counts), st), "mc_raw_hot_detect")
        hot_keys, order = torch.sort(keys[:n], stable=True)
        hot_rv = rv[:n][order].contiguous()
        check(lib.mc_raw_hot_finalize(ptr(hot_keys), ptr(hot_rv), n, t, h, w, hl, hu, wl, wu, 1, ptr(hstats),
                                      ptr(stats), ptr(mu), ptr(sub), ptr(mean_rstd), st), "mc_raw_hot_finalize")
        return hot_keys, hot_rv, counts, counter, mu, sub, mean_rstd

    return make, route


@case("global raw 512 with hot pixels", ["mc_xc_rows_forward_raw", "mc_xc_rows_hot_correct"])
def _():
    return (lambda dev: dict(rm=_raw(3, 512, 512, True, dev)),
            lambda rm: E().global_shifts_raw(rm, 1, 1.0, BF, BAND))


@case("global raw 96 x 5760", ["mc_xcg_rows_forward_raw"])
def _():
    return (lambda dev: dict(rm=_raw(2, 96, 5760, False, dev)),
            lambda rm: E().global_shifts_raw(rm, 0, 1.0, BF, BAND))


@case("rigid warp 61 x 67", ["mc_spline_lattice", "mc_warp_rigid_phase_t"])
def _():
    def route(img, field):
        lat = E().frame_lattices(field, img.shape[0], "catmull_rom")
        return E().warp(img, lat, 1.0, want_frames=True, want_sum=True, rigid=True)

    return (lambda dev: dict(img=float_stack(3, 61, 67).to(dev), field=_rigid_field(3, dev)), route)


def _local_field(t, dev):
    g = torch.Generator().manual_seed(t + 3)
    return ((torch.rand(2, t, 2, 2, generator=g) - 0.5) * 4.0).to(dev)


@case("field warp 130 x 257", ["mc_warp_frames_t", "mc_pixel_shifts", "mc_pixel_shifts_at"])
def _():
    def route(img, field, coords):
        t, h, w = img.shape
        lat = E().frame_lattices(field, t, "catmull_rom")
        return (E().warp(img, lat, 1.0, want_frames=True, want_sum=True), E().pixel_shifts(lat[0], h, w, 1.0),
                E().pixel_shifts_at(lat[1], h, w, 1.0, coords))

    def make(dev):
        g = torch.Generator().manual_seed(4)
        coords = torch.rand(37, 2, generator=g) * torch.tensor([129.0, 256.0])
        return dict(img=float_stack(3, 130, 257).to(dev), field=_local_field(3, dev), coords=coords.to(dev))

    return make, route


@case("rigid tables from shifts", ["mc_rigid_tables_from_shifts"])
def _():
    def route(img, shifts):
        field, tables = E().rigid_tables_from_shifts(shifts, img.shape, 1.0, "catmull_rom")
        return field, E().warp(img, None, 1.0, want_frames=True, want_sum=True, rigid=True, tables=tables)

    return (lambda dev: dict(img=float_stack(3, 61, 67).to(dev), shifts=_shifts(3, dev)), route)


@case("raw rigid warp 256 x 256 with hot pixels", ["mc_warp_rigid_raw", "mc_warp_rigid_raw_accumulate",
                                                    "mc_warp_rigid_hot_taps", "mc_hot_scatter_add"])
def _():
    def route(rm, field, base):
        lat = E().frame_lattices(field, rm.shape[0], "catmull_rom")
        acc = base.clone()
        return (E().warp_rigid_raw(rm, lat, 1.0, want_frames=True, want_sum=True),
                E().warp_rigid_raw(rm, lat, 1.0, want_frames=False, out_sum=acc, accumulate=True))

    return (lambda dev: dict(rm=_raw(3, 256, 256, True, dev), field=_rigid_field(3, dev),
                             base=float_stack(1, 256, 256)[0].to(dev)), route)


@case("raw field warp 512 x 256", ["mc_warp_frames_raw", "mc_warp_frames_raw_accumulate"])
def _():
    def route(rm, field, base):
        lat = E().frame_lattices(field, rm.shape[0], "catmull_rom")
        acc = base.clone()
        return (E().warp_field_raw(rm, lat, 1.0, want_frames=True, want_sum=True),
                E().warp_field_raw(rm, lat, 1.0, want_frames=False, out_sum=acc, accumulate=True))

    # (the raw field kernel stages at most 1.5 lattice cells per 32 pixel rows: 20 lattice rows need h >= 407)
    return (lambda dev: dict(rm=_raw(3, 512, 256, False, dev), field=_local_field(3, dev),
                             base=float_stack(1, 512, 256)[0].to(dev)), route)


@case("conditioning", ["mc_condition_movie", "mc_condition_movie_hot"], rel=ATOMIC_REL)
def _():
    return (lambda dev: dict(raw=_hot_movie(3, 128, 96, 6).to(dev), g=gain(128, 96).to(dev)),
            lambda raw, g: (E().condition_movie(raw, g), E().condition_movie(raw, g, hot_pixel_threshold=10.0)))


@case("frame groups, frame sum", ["mc_raw_group_frames", "mc_sum_frames"])
def _():
    return (lambda dev: dict(raw=raw_movie(5, 64, 96, torch.int16, 8).to(dev), img=float_stack(3, 64, 96).to(dev)),
            lambda raw, img: (E().sum_frames(img), E().group_frames_raw(raw, 3)))  # the flag's read-back comes last


@case("normalise (on S: the negative control's other half)", ["mc_normalize"])
def _():
    return (lambda dev: dict(img=float_stack(3, 61, 67).to(dev),
                             stats=torch.tensor([5.0, 0.5, 2.0], dtype=torch.float32, device=dev)),
            lambda img, stats: E().normalize(img, stats))


@case("plan tables", ["mc_circle_mask", "mc_xc_filter"])
def _():
    def route(dev):
        from torch_motion_correction_amd import _lib, plan
        from torch_motion_correction_amd._lib import check, ptr, stream_ptr

        mask = plan.circle_mask(96, 160, 24.0, 12.0, dev)
        low, high = plan.band_limits(BAND, 1.0)
        geom = plan.xc_geometry(96, 160, high, 24.0, 12.0)
        filt = torch.empty((geom.nkx, geom.nky), dtype=torch.float32, device=dev)
        check(_lib.load().mc_xc_filter(ptr(filt), geom, low, high, BF, 1.0, stream_ptr(dev)), "mc_xc_filter")
        return mask, filt

    return (lambda dev: dict(dev=dev), route)


@case("patch jobs 1024, wave-per-row", ["mc_xc_rows_forward_dual_t"])
def _():
    def make(dev):
        p, jobs = 1024, [(0, 1, 3), (1, 7, 13), (0, 9, 5), (1, 0, 1)]
        H, W = p + 9, p + 14
        x = xr.noise(2, H, W, mean=5.0, std=2.0)
        off = [f * H * W + y * W + c for f, y, c in jobs]
        return dict(x=x.to(dev), off=torch.tensor(off, dtype=torch.int64, device=dev),
                    ea=torch.tensor([1, 2, 3, 1], dtype=torch.int32, device=dev),
                    eb=torch.tensor([2, 4, 6, 2], dtype=torch.int32, device=dev),
                    stats=torch.tensor([5.0, 0.5, 2.0], dtype=torch.float32, device=dev))

    def route(x, off, ea, eb, stats):
        from torch_motion_correction_amd import plan

        pl = plan.get_xc_plan(1024, 1024, 1.0, BF, BAND, x.device)
        return E()._forward_spectra(x, off, x.shape[2], ea, pl, stats, job_expo_b=eb, min_expo=1)

    return make, route


@case("raw patch jobs 16 x 1024", ["mc_xc_rows_forward_dual_raw"])
def _():
    def make(dev):
        raw, g = xr.raw_patch_input("u8", 16)
        rm = E().RawMovie(raw.to(dev), g.to(dev))
        ea, eb = (torch.tensor(e, dtype=torch.int32, device=dev) for e in xr.RAW_PATCH_EXPO)
        return dict(rm=rm, off=torch.tensor(xr.check_raw_patch_jobs(16), dtype=torch.int64, device=dev), ea=ea, eb=eb,
                    frames=torch.tensor([f for f, _, _ in xr.RAW_PATCH_JOBS], dtype=torch.int64, device=dev))

    def route(rm, off, ea, eb, frames):
        from torch_motion_correction_amd import plan

        pl = plan.get_xc_plan(16, 1024, 1.0, BF, BAND, off.device)
        return E().raw._patch_spectra_raw(rm, pl)(off, ea, frames, eb, min_expo=1)  # frames on the device: no upload

    return make, route


@case("local-motion loss sums", ["mc_local_loss_sums", "mc_local_ncc_grad"])
def _():
    def make(dev):
        from torch_motion_correction_amd import local_motion

        img = float_stack(3, 130, 257).to(dev)
        prob = local_motion.LocalMotionProblem(img, 1.0, (48, 48), (2, 2, 2), "catmull_rom")
        g = torch.Generator().manual_seed(12)
        return dict(prob=prob, s=((torch.rand(prob.npatch, 3, 2, generator=g) - 0.5) * 3).to(dev),
                    ab=torch.rand(prob.npatch, 3, 2, generator=g).to(dev))

    return make, lambda prob, s, ab: (prob.sums(s, True), prob.sums(s, False), prob.ncc_grad_sums(s, ab))


@case("magnification 61 x 67", ["mc_affine_resample", "mc_affine_warp_sum"])
def _():
    def route(img, shifts):
        from torch_motion_correction_amd import magnification as mg

        m = mg.magnification_distortion_matrix(1.02, 0.98, 30.0)
        return mg._resample(img, m, 0.0), mg._warp_sum(img, E().STORE_F32, None, None, m, shifts, True)

    return (lambda dev: dict(img=float_stack(3, 61, 67).to(dev), shifts=_shifts(3, dev)), route)


@case("calibration sums, defect fill", ["mc_raw_pixel_sums", "mc_defect_donors", "mc_raw_fill_defects",
                                        "mc_gain_fill_defects"])
def _():
    def make(dev):
        from torch_motion_correction_amd import calibration

        dmap = torch.zeros(64, 96, dtype=torch.bool)
        dmap[5, 7] = dmap[5, 8] = dmap[40, :] = dmap[63, 95] = True
        fill = calibration.DefectFill(dmap.to(dev))
        return dict(raw=raw_movie(3, 64, 96, torch.uint8, 2).to(dev), g=gain(64, 96).to(dev), fill=fill,
                    dmap=dmap.to(dev).view(torch.uint8))

    def route(raw, g, fill, dmap):
        from torch_motion_correction_amd import _lib, calibration
        from torch_motion_correction_amd._lib import check, ptr, stream_ptr

        st = calibration.RawStatistics((64, 96)).add(raw)
        # DefectFill.__init__ lists the defects with torch.nonzero (a read-back); the launch itself, on that list:
        donors = torch.empty((fill.n, 8 * fill.reach), dtype=torch.int32, device=raw.device)
        counts = torch.empty((fill.n,), dtype=torch.int32, device=raw.device)
        check(_lib.load().mc_defect_donors(ptr(dmap), 64, 96, ptr(fill.pixels), fill.n, fill.reach, ptr(donors),
                                           ptr(counts), stream_ptr(raw.device)), "mc_defect_donors")
        return (st.sum, st.sumsq, donors, counts, calibration.fill_defects_raw(raw, fill, seed=7),
                calibration.fill_defects_gain(g, fill))

    return make, route


@case("MRC decode, orient, encode", ["mc_mrc_decode", "mc_raw_orient", "mc_mrc_encode"])
def _():
    def route(data, movie):
        from torch_motion_correction_amd import mrc

        return (mrc._decode(data, 8, 2, 30, 50, 1, False, False, True, None),
                mrc._orient(movie, 1, mrc._FLIPS["ud"], None),
                mrc._encode(movie, 3, 64, 96, 1, True, None)[0])  # (the statistics' read-back comes last)

    def make(dev):
        g = torch.Generator().manual_seed(21)
        return dict(data=torch.randint(0, 256, (8 + 2 * 30 * 50 * 2,), dtype=torch.uint8, generator=g).to(dev),
                    movie=raw_movie(3, 64, 96, torch.int16, 4).to(dev))

    return make, route


@case("TIFF encode and pack", ["mc_tiff_encode", "mc_tiff_pack"])
def _():
    def make(dev):
        from torch_motion_correction_amd import tiff

        movie = raw_movie(2, 64, 96, torch.uint8, 11).to(dev)
        _, _, produced = tiff._encode_strips(movie.reshape(-1), 2, 4, 64, 96, 16, dev)
        return dict(movie=movie, total=int(produced.sum()))

    def route(movie, total):
        from torch_motion_correction_amd import tiff

        dev = movie.device
        slots, slot, produced = tiff._encode_strips(movie.reshape(-1), 2, 4, 64, 96, 16, dev)
        return produced, tiff._pack_strips(slots, slot, produced, total, dev)

    return make, route


def _lib3():
    from torch_motion_correction_amd import _lib
    from torch_motion_correction_amd._lib import check, ptr, stream_ptr

    return _lib.load(), check, ptr, stream_ptr


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# The six entry points below sit, in their Python routes (engine._patch_field_core, engine.refine_patch_shifts,
# engine.spline_points), behind per-call uploads of index tables from host memory, which wait for the stream as a
# read-back does.  They are called through `lib`, on the hand-built device tables of their float64 tests
# (post_reference, iteration_reference, test_xc_kernels_float64's accumulate input), staged in make().


@case("leave-one-out reference spectra (direct)", ["mc_xc_ref_mean_except_current"])
def _():
    import post_reference as pr

    def make(dev):
        from torch_motion_correction_amd import lattice

        t, npatch, length = 8, 3, 173
        table = lattice.mask_schedule(t, "mean_except_current", t // 2)[0]
        sp, si, sr = (_t(a, dev) for a in lattice.leave_one_out_schedule(table))
        u, v = pr.ref_inputs(t, npatch, length, "independent")
        return dict(u=_t(u, dev), v=_t(v, dev), sp=sp, si=si, sr=sr)

    def route(u, v, sp, si, sr):
        lib, check, ptr, stream_ptr = _lib3()
        t, npatch, length, _ = u.shape
        ref = torch.empty_like(u)
        check(lib.mc_xc_ref_mean_except_current(ptr(u), ptr(v), ptr(sp), ptr(si), ptr(sr), ptr(ref), t, npatch, length,
                                                1.0 / (t - 1), stream_ptr(u.device)), "mc_xc_ref_mean_except_current")
        return ref

    return make, route


@case("field accumulate, smooth and centre (direct)", ["mc_field_accumulate", "mc_field_smooth_center"])
def _():
    P, npatch, t, frames = 64, 10, 5, [3, 0, 4]

    def make(dev):
        rng = np.random.default_rng(11)
        nf = len(frames)
        nb = rng.uniform(0.2, 0.8, size=(nf * npatch, 3, 3)).astype(np.float32)
        nb[:, 1, 1] = 1.5 + rng.uniform(0, 0.5, size=nf * npatch).astype(np.float32)
        peaks = (rng.integers(1, P - 1, nf * npatch) * P + rng.integers(1, P - 1, nf * npatch)).astype(np.int32)
        return dict(peaks=_t(peaks, dev), nb=_t(nb, dev), fr=_t(np.asarray(frames, dtype=np.int32), dev),
                    field0=_t(rng.standard_normal((2, t, npatch)).astype(np.float32), dev))

    def route(peaks, nb, fr, field0):
        lib, check, ptr, stream_ptr = _lib3()
        st = stream_ptr(nb.device)
        field = field0.clone()  # accumulated in place
        check(lib.mc_field_accumulate(ptr(peaks), ptr(nb), ptr(fr), len(frames), npatch, P, t, 1.3, 5.0, 3, ptr(field),
                                      st), "mc_field_accumulate")
        out = torch.empty_like(field)
        check(lib.mc_field_smooth_center(ptr(field), ptr(out), t, npatch, 3, 1, st), "mc_field_smooth_center")
        return field, out

    return make, route


@case("patch refinement kernels (direct)", ["mc_xc_aligned_refs_patches", "mc_xc_refine_update_patches"])
def _():
    import iteration_reference as ir

    acase, (H, W), under, t = (6, 5, 9, 16), (96, 120), 16, 6

    def make(dev):
        a = ir.aligned_patch_case(acase)
        u = ir.update_patch_case(t, 1, (H, W), under, 0, ir.NPATCH)
        return dict(S=_t(a["S"], dev), sh=_t(a["shifts"], dev), of=_t(a["offsets"], dev), fy=_t(a["fy"], dev),
                    fx=_t(a["fx"], dev), peaks=_t(u["peaks"], dev), nb=_t(u["nb"], dev), ush=_t(u["shifts"], dev),
                    max_r=_t(u["max_r"], dev), ref=int(u["ref"]))

    def route(S, sh, of, fy, fx, peaks, nb, ush, max_r, ref):
        lib, check, ptr, stream_ptr = _lib3()
        st = stream_ptr(S.device)
        ta, nkx, nky, und = acase
        nq = ir.NPATCH
        G = torch.empty((ta, nq, nkx, nky, 2), dtype=torch.float32, device=S.device)
        REF = torch.empty_like(G)
        check(lib.mc_xc_aligned_refs_patches(ptr(S), ptr(sh), ptr(of), ptr(fy), ptr(fx), ptr(G), ptr(REF), ta, nq, 0,
                                             nq, nkx, nky, und, st), "mc_xc_aligned_refs_patches")
        s, m = ush.clone(), max_r.clone()  # updated in place
        check(lib.mc_xc_refine_update_patches(ptr(peaks), ptr(nb), ptr(s), ref, t, nq, 0, nq, H, W, under, ptr(m), st),
              "mc_xc_refine_update_patches")
        return G, REF, s, m

    return make, route


@case("spline points (direct)", ["mc_spline_points"])
def _():
    def make(dev):
        from torch_motion_correction_amd import spline

        field = _local_field(3, dev)
        pts = torch.rand(23, 3, generator=torch.Generator().manual_seed(31))
        tabs = [spline.axis_taps(size, pts[:, a].contiguous(), "catmull_rom") for a, size in enumerate(field.shape[1:])]
        taps = {f"{k}{a}": x.to(dev) for a, (i, w) in enumerate(tabs) for k, x in (("i", i), ("w", w))}
        return dict(field=field, **taps)

    def route(field, i0, w0, i1, w1, i2, w2):
        lib, check, ptr, stream_ptr = _lib3()
        c, nt, nh, nw = field.shape
        n = int(i0.shape[0])
        out = torch.empty((n, c), dtype=torch.float32, device=field.device)
        check(lib.mc_spline_points(ptr(field), c, nt, nh, nw, ptr(i0), ptr(w0), ptr(i1), ptr(w1), ptr(i2), ptr(w2), n,
                                   ptr(out), stream_ptr(field.device)), "mc_spline_points")
        return out

    return make, route


@case("TIFF decode", [], after=["mc_tiff_decode"])
def _():
    def make(dev):
        from torch_motion_correction_amd import tiff

        movie = raw_movie(2, 64, 96, torch.uint8, 11).to(dev)
        slots, slot, produced = tiff._encode_strips(movie.reshape(-1), 2, 4, 64, 96, 16, dev)
        n = [int(v) for v in produced.tolist()]
        payload = tiff._pack_strips(slots, slot, produced, sum(n), dev)
        return dict(data=payload, offs=tuple(int(v) for v in np.cumsum([0] + n[:-1])), n=tuple(n))

    def route(data, offs, n):
        from torch_motion_correction_amd import tiff

        return tiff._decode_strips(data, list(offs), list(n), 2, 4, 64, 96, 16, 5, None)

    return make, route


@case("EER render", [], after=["mc_eer_render"])
def _():
    def make(dev):
        import eer_reference as er

        r = np.random.default_rng(5)
        strips = [er.encode_frame(*er.random_frame(r, 32 * 48, 0.05), 32 * 48) for _ in range(4)]
        buf, offs, n = er.lay_out(strips, None)
        return dict(data=torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev), offs=tuple(offs), n=tuple(n))

    def route(data, offs, n):
        from torch_motion_correction_amd import eer

        return eer._render(data, list(offs), list(n), 32, 48, 2, 1, None)

    return make, route
