"""Host checks of tests/post_reference.py -- the float64 definitions, bounds and case lists behind
tests/test_post_kernels_float64.py -- without a GPU: every definition against the project's fp32 CPU oracle (oracle/,
scipy.signal.savgol_filter, scipy.ndimage.distance_transform_edt) INSIDE the bound of every case (a bound the oracle
broke would be a wrong bound), the host halves of the kernels (lattice.leave_one_out_schedule, spline.axis_taps) replayed
in fp32 on the CPU against the same bounds, the branch each case is there to reach, and the argument rules of the five
entry points, which return before any launch.

The oracle's worst error / bound per family is printed as `RATIO ...` (run with -s); those figures are the last column
of the table in tests/test_post_kernels_float64.py."""

import ctypes

import numpy as np
import pytest
import torch
from scipy.signal import savgol_filter

import post_reference as pr
from oracle import motion as om
from oracle import thirdparty_semantics as tp
from torch_motion_correction_amd import _lib, lattice, plan, spline

U = pr.U
F32 = np.float32


# ------------------------------------------------------------------ A. reference spectra


def _table(name):
    if isinstance(name, int):
        return lattice.mask_schedule(name, "mean_except_current", name // 2)[0]
    return pr.hand_table(pr.HAND_TABLES[name])


def _replay(u, v, sched, t, dtype):
    """The kernel's arithmetic from the host schedule, in `dtype`: T, the running d, ((T - U_f) + d) * inv."""
    ptr, idx, rebuild = sched
    u, v = u.astype(dtype), v.astype(dtype)
    T = np.zeros_like(u[0])
    for o in range(t):
        T = T + u[o]
    inv = dtype(1.0 / (t - 1))
    d = np.zeros_like(T)
    out = np.empty_like(u)
    for f in range(t):
        if rebuild[f]:
            d = np.zeros_like(T)
        for q in range(ptr[f], ptr[f + 1]):
            d = d + (v[idx[q]] - u[idx[q]])
        out[f] = ((T - u[f]) + d) * inv
    return out


def _oracle_ref(u, v, table):
    """The oracle's own fp32 sequence (oracle.motion, the mean_except_current loop): clone the first, += the others
    in frame order, / n."""
    t = u.shape[0]
    ut, vt = torch.from_numpy(u), torch.from_numpy(v)
    out = torch.empty_like(ut)
    for f in range(t):
        acc, n = None, 0
        for o in range(t):
            if o == f:
                continue
            other = vt[o] if table[f, o] == 1 else ut[o]
            acc = other.clone() if acc is None else acc.add_(other)
            n += 1
        out[f] = acc / n
    return out.numpy()


TABLES = pr.SCHEDULE_T + list(pr.HAND_TABLES)


@pytest.mark.parametrize("pair", pr.REF_PAIRS)
@pytest.mark.parametrize("name", TABLES)
def test_reference_spectra_definition_schedule_and_oracle(name, pair):
    table = _table(name)
    t = table.shape[0]
    sched = lattice.leave_one_out_schedule(table)
    assert sched[0].dtype == np.int32 and sched[1].dtype == np.int32 and sched[2].dtype == np.uint8
    assert len(sched[0]) == t + 1 and len(sched[2]) == t and sched[0][-1] <= len(sched[1]) and len(sched[1]) >= 1
    assert ((0 <= sched[1]) & (sched[1] < t)).all()
    worst_o = worst_k = 0.0
    for npatch, length in (pr.REF_SIZES if name == 8 else pr.REF_SIZES[-1:]):
        u, v = pr.ref_inputs(t, npatch, length, pair)
        ref, bound = pr.ref_mean64(pr.to_complex(u), pr.to_complex(v), table)
        flat = lambda a: a.reshape(t, -1, 2)  # noqa: E731
        want = np.stack([ref.real, ref.imag], axis=-1)
        # the host schedule replays the table exactly (float64), and in fp32 stays inside the bound
        exact = _replay(flat(u), flat(v), sched, t, np.float64)
        assert np.abs(exact - want).max() <= 1e-12 * t
        worst_k = max(worst_k, float((np.abs(_replay(flat(u), flat(v), sched, t, F32).astype(np.float64) - want) / bound).max()))
        worst_o = max(worst_o, float((np.abs(_oracle_ref(flat(u), flat(v), table).astype(np.float64) - want) / bound).max()))
        if pair == "independent":
            sens = pr.ref_sensitivity(pr.to_complex(u), pr.to_complex(v), bound)
            assert sens >= 100, f"table {name} size {npatch} x {length}: one swapped member moves the reference by {sens:.1f} bounds"
        else:
            print(f"  table {name} size {npatch} x {length} masked pair: smallest sensitivity {pr.ref_sensitivity(pr.to_complex(u), pr.to_complex(v), bound):.2f} bounds")
    print(f"RATIO ref_mean_except_current table {name} {pair}: oracle {worst_o:.3f} fp32 replay of the schedule {worst_k:.3f}")
    assert worst_o < 1 and worst_k < 1


@pytest.mark.parametrize("t", [52, 60])
def test_long_tables_reach_a_rebuild_and_go_on_adding(t):
    _, _, rebuild = lattice.leave_one_out_schedule(_table(t))
    later = np.nonzero(rebuild[1:])[0] + 1
    assert len(later) >= 1, "no memo eviction"
    assert (rebuild[later[0] + 1:] == 0).any(), "no incremental frame after the rebuild"


@pytest.mark.parametrize("t", [2, 3, 8])
def test_short_tables_add_one_frame_per_step(t):
    ptr, idx, rebuild = lattice.leave_one_out_schedule(_table(t))
    assert rebuild.tolist() == [1] + [0] * (t - 1) and np.diff(ptr).tolist() == [0] + [1] * (t - 1)


def test_hand_tables_reach_their_branches():
    reb = {k: lattice.leave_one_out_schedule(_table(k))[2].tolist() for k in pr.HAND_TABLES}
    assert reb["reset"] == [1, 0, 0, 1, 0, 0]           # S_3 is no superset of S_2
    assert reb["empty"] == [1, 0, 0, 0] and np.diff(lattice.leave_one_out_schedule(_table("empty"))[0]).tolist() == [0] * 4
    assert reb["full"] == [1] * 5                        # every frame is a member of its predecessor's set
    sets = pr.HAND_TABLES["member"]
    assert 1 in sets[0] and 3 not in sets[2] and reb["member"] == [1, 1, 1, 0, 1]
    assert sets[2] <= sets[3] and not sets[3] <= sets[4]  # frame 3 adds {4}; frame 4 (a member of S_3) rebuilds
    assert sum(len(s) for s in pr.HAND_TABLES["full"]) == 20


def test_sizes_end_in_a_partial_block():
    assert [n * l for n, l in pr.REF_SIZES] == [1, 255, 257, 519]
    assert all((n * l) % 256 for n, l in pr.REF_SIZES) and pr.REF_SIZES[-1][0] > 1


# ------------------------------------------------------------------ B. smoothing


@pytest.mark.parametrize("t", pr.SAVGOL_T)
def test_smoothing_definition_is_scipys_filter(t):
    x = pr.smooth_field(t, 6, "unit").astype(np.float64)
    for window in range(3, t + 1):
        want = savgol_filter(x, window, 1, axis=1)
        got, _ = pr.smooth64(x, window, 0)
        assert np.abs(got - want).max() <= 1e-12, (t, window)
    assert np.array_equal(pr.smooth64(x, 0, 0)[0], x)


def _oracle_smooth(x, window, subtract_mean):
    """The contract with fp32 storage and double accumulation, by the oracle's own calls: scipy's filter on the fp32
    series widened to float64, rounded to fp32 once; then `field - mean(field)` with the mean taken in double and
    rounded once, the difference in fp32.  The oracle's literal fp32 forms are NOT inside these bounds and are not
    meant to be: scipy on an fp32 array forms coefficients and edge fits in fp32 (up to 12 bounds where the smoothed
    value cancels), torch.mean on fp32 accumulates in fp32 (up to 10 bounds on a field whose mean is near 0) -- the
    two reasons the kernel accumulates in double, and the second is one of the mutations the GPU file lists."""
    y = torch.from_numpy(np.asarray(savgol_filter(x.astype(np.float64), window, 1, axis=1), dtype=F32)) if window >= 3 \
        else torch.from_numpy(x.copy())
    return (y - y.double().mean().float()).numpy() if subtract_mean else y.numpy()


@pytest.mark.parametrize("kind", ["unit", "mean1000", "grid1000"])
@pytest.mark.parametrize("npatch", pr.SMOOTH_NPATCH)
def test_oracle_smoothing_is_inside_the_bound(npatch, kind):
    worst = 0.0
    for t in pr.SMOOTH_T:
        x = pr.smooth_field(t, npatch, kind)
        for window in pr.smooth_windows(t):
            for sub in (0, 1):
                want, bound = pr.smooth64(x, window, sub)
                err = np.abs(_oracle_smooth(x, window, sub).astype(np.float64) - want)
                ok = bound > 0
                assert (err[~ok] == 0).all()
                if ok.any():
                    worst = max(worst, float((err[ok] / bound[ok]).max()))
    print(f"RATIO field_smooth_center npatch {npatch} {kind}: oracle {worst:.3f}")
    assert worst < 1


def test_series_loop_trips():
    trips = {n: -(-2 * n // 256) for n in pr.SMOOTH_NPATCH}
    assert trips == {1: 1, 6: 1, 127: 1, 129: 2, 300: 3} and 2 * 129 > 256 and 2 * 300 > 512


def test_an_fp32_mean_misses_the_bound_on_the_grid_field():
    """The stand-in for a kernel that accumulates the mean in fp32 (256 threads, fp32 partial sums) is outside the
    bound on 'grid1000' at (t, npatch) = (40, 300), and inside it on the plain N(1000, 1) field: that is why the grid
    field is a case."""
    x = pr.smooth_field(40, 300, "grid1000")
    want, bound = pr.smooth64(x, 0, 1)
    got = (x - F32(pr.fp32_mean_by_threads(x))).astype(np.float64)
    assert (np.abs(got - want) / bound).max() > 3
    x = pr.smooth_field(40, 300, "mean1000")
    want, bound = pr.smooth64(x, 0, 1)
    got = (x - F32(pr.fp32_mean_by_threads(x))).astype(np.float64)
    print(f"  fp32 mean on N(1000, 1): {(np.abs(got - want) / bound).max():.3f} bounds")


# ------------------------------------------------------------------ C. spline grids


def _fp32_taps_lattice(data, q, grid_type):
    """spline.axis_taps' tables evaluated as the kernel does: three nested fp32 sums, x then y then t."""
    tabs = [spline.axis_taps(n, torch.from_numpy(np.asarray(u, dtype=F32)), grid_type) for n, u in zip(data.shape[1:], q)]
    (it, wt), (iy, wy), (ix, wx) = [(i.numpy().astype(np.int64), w.numpy()) for i, w in tabs]
    d = data[:, :, :, ix]                                   # (c, nt, nh, NX, 4)
    vx = np.zeros(d.shape[:-1], dtype=F32)
    for k in range(4):
        vx = (vx + (d[..., k] * wx[:, k]).astype(F32)).astype(F32)
    d = np.moveaxis(vx[:, :, iy], (2, 3), (3, 4))           # (c, nt, NX, NY, 4)
    vy = np.zeros(d.shape[:-1], dtype=F32)
    for k in range(4):
        vy = (vy + (d[..., k] * wy[:, k]).astype(F32)).astype(F32)
    d = np.moveaxis(vy[:, it], (1, 2), (3, 4))              # (c, NX, NY, NT, 4)
    vt = np.zeros(d.shape[:-1], dtype=F32)
    for k in range(4):
        vt = (vt + (d[..., k] * wt[:, k]).astype(F32)).astype(F32)
    return np.transpose(vt, (0, 3, 2, 1))                   # (c, NT, NY, NX)


def _oracle_lattice(data, q, grid_type):
    ut, uy, ux = (torch.from_numpy(np.asarray(u, dtype=F32)) for u in q)
    g = torch.stack(torch.meshgrid(ut, uy, ux, indexing="ij"), dim=-1)
    return tp.cubic_spline_grid_3d(torch.from_numpy(data), g, grid_type).permute(3, 0, 1, 2).numpy()


@pytest.mark.parametrize("grid_type", pr.GRID_TYPES)
@pytest.mark.parametrize("shape", pr.SPLINE_GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_spline_lattice_oracle_and_host_taps_inside_the_bound(shape, grid_type):
    worst_o = worst_k = 0.0
    for kind in pr.SPLINE_QUERIES:
        data, q, val, bound = pr.lattice_case(shape, kind, grid_type)
        assert val.shape == (shape[0], len(q[0]), len(q[1]), len(q[2])) and (bound > 0).all()
        worst_o = max(worst_o, float((np.abs(_oracle_lattice(data, q, grid_type).astype(np.float64) - val) / bound).max()))
        worst_k = max(worst_k, float((np.abs(_fp32_taps_lattice(data, q, grid_type).astype(np.float64) - val) / bound).max()))
    print(f"RATIO spline lattice {shape} {grid_type}: oracle {worst_o:.3f} fp32 replay of axis_taps {worst_k:.3f}")
    assert worst_o < 1 and worst_k < 1


@pytest.mark.parametrize("grid_type", pr.GRID_TYPES)
@pytest.mark.parametrize("shape", pr.SPLINE_GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_spline_points_oracle_inside_the_bound(shape, grid_type):
    worst = 0.0
    for n in pr.POINT_COUNTS:
        data, pts, val, bound = pr.points_case(shape, n, grid_type)
        got = tp.cubic_spline_grid_3d(torch.from_numpy(data), torch.from_numpy(pts), grid_type).numpy()
        worst = max(worst, float((np.abs(got.astype(np.float64) - val) / bound).max()))
        if n >= 8:
            assert sorted(map(tuple, pts[:8].tolist())) == [(i, j, k) for i in (0., 1.) for j in (0., 1.) for k in (0., 1.)]
    print(f"RATIO spline points {shape} {grid_type}: oracle {worst:.3f}")
    assert worst < 1


def test_lattice_and_point_definitions_agree():
    shape = (3, 7, 6, 9)
    data = pr.spline_grid(shape)
    pts = pr.spline_points(shape, 257)
    pv, _ = pr.spline_points64(data, pts, "bspline")
    for i in (0, 7, 100, 256):
        lv, _ = pr.spline_lattice64(data, pts[i:i + 1, 0], pts[i:i + 1, 1], pts[i:i + 1, 2], "bspline")
        assert np.abs(lv[:, 0, 0, 0] - pv[i]).max() <= 1e-12


def test_cases_reach_both_folds_the_end_intervals_and_u_equal_one():
    il2, _ = pr.intervals(2, pr.edge_vector(2))
    assert (il2 == 0).all()                                  # n = 2: il == 0 and il + 2 == n on every query: both folds
    il1, _ = pr.intervals(1, pr.edge_vector(1))
    assert (il1 == 0).all()                                  # a single sample: duplicated, the same
    ev = pr.edge_vector(3)
    il3, s3 = pr.intervals(3, ev)
    assert set(il3.tolist()) == {0, 1}                       # n = 3: lo fold in the first, hi fold in the last interval
    one = ev == 1.0
    assert one.any() and (il3[one] == 1).all() and (s3[one] == 1.0).all()   # u == 1: the last interval at s = 1
    k = pr.knots32(3).numpy()[1]
    below, at, above = (ev == np.nextafter(k, F32(0))), (ev == k), (ev == np.nextafter(k, F32(1)))
    assert (il3[below] == 0).all() and (il3[at] == 1).all() and (s3[at] == 0).all() and (il3[above] == 1).all()
    assert any(s[1] == 2 or s[2] == 2 or s[3] == 2 for s in pr.SPLINE_GRIDS) and any(3 in s[1:] for s in pr.SPLINE_GRIDS)
    sizes = [int(np.prod([shape[0]] + [len(u) for u in pr.spline_query(shape, kind)]))
             for shape in pr.SPLINE_GRIDS for kind in pr.SPLINE_QUERIES]
    assert any(n % 256 and n > 1024 for n in sizes) and min(sizes) < 256
    assert all((n * c) % 256 for n in pr.POINT_COUNTS for c in (1, 2, 3) if n != 256)


@pytest.mark.parametrize("shape", pr.SPLINE_GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_catmull_rom_interpolates_its_samples(shape):
    data = pr.spline_grid(shape)
    q = tuple(pr.knots32(n).numpy()[:n] if n > 1 else np.zeros(1, dtype=F32) for n in shape[1:])
    val, bound = pr.spline_lattice64(data, *q, "catmull_rom")
    assert (np.abs(val - data) <= bound).all()


# ------------------------------------------------------------------ D. plan tables


@pytest.mark.parametrize("case", pr.MASK_CASES, ids=lambda c: "-".join(f"{v:g}" for v in c))
def test_mask_definition_is_the_oracles_circle(case):
    h, w, r, s = case
    inside, ring, value, _ = pr.mask64(*case)
    if not inside.any():
        assert r == 0 and not value.any()  # scipy's transform has no background to measure to: mcorr.h says zeros
        return
    got = tp.circle(r, (h, w), smoothing_radius=s).numpy()
    assert (got[inside] == 1).all() and (got[~inside & ~ring] == 0).all()
    err = np.abs(got.astype(np.float64) - value)[ring]
    if ring.any():
        print(f"RATIO circle mask {case}: oracle {err.max() / pr.MASK_RING_BOUND:.3f} ({int(ring.sum())} ring pixels)")
        assert err.max() < pr.MASK_RING_BOUND
        assert ((value[ring] >= 0) & (value[ring] < 1)).all()


def test_mask_cases_reach_the_clamps_and_several_blocks():
    reach = {}
    for case in pr.MASK_CASES:
        h, w, r, s = case
        inside, ring, _, halfw = pr.mask64(*case)
        cx = w // 2
        reach[case] = dict(right=bool((cx + halfw[halfw >= 0] > w - 1).any()), left=bool((cx - halfw[halfw >= 0] < 0).any()),
                           ring_cut=bool(ring[:, [0, -1]].any() or ring[[0, -1]].any()),
                           disk_cut_y=bool(inside[[0, -1]].any()), yblocks=-(-h // 64), xblocks=-(-w // 256))
    assert reach[(40, 24, 16, 4)]["right"] and reach[(40, 24, 16, 4)]["left"]
    assert reach[(32, 48, 12, 12)]["ring_cut"] and not reach[(32, 48, 12, 12)]["disk_cut_y"]
    assert reach[(32, 96, 24, 24)]["disk_cut_y"]
    assert reach[(64, 300, 16, 8)]["xblocks"] == 2 and reach[(100, 120, 25, 12.5)]["yblocks"] == 2
    assert reach[(130, 66, 16.5, 8.25)]["yblocks"] == 3 and reach[(121, 135, 30.25, 15.125)]["yblocks"] == 2
    assert pr.mask64(16, 16, 0.5, 3)[0].sum() == 1 and not pr.mask64(24, 40, 0, 5)[0].any()
    assert any(float(r) != int(r) for _, _, r, _ in pr.MASK_CASES)


def filter_args(case):
    H, W, ps, B, band, _ = case
    low, high = plan.band_limits(band, ps)
    g = plan.xc_geometry(H, W, high, min(H, W) / 4, min(H, W) / 8)
    return g, low, high


@pytest.mark.parametrize("case", pr.FILTER_CASES, ids=lambda c: c[5])
def test_filter_definition_is_the_oracles_and_the_plan_prunes_nothing_kept(case):
    H, W, ps, B, band, what = case
    g, low, high = filter_args(case)
    kept, value, bound = pr.filter64(W, H, g.nkx, g.kyp, g.kyn, low, high, B, ps)
    _, benv, bandf = om._filters((H, W), ps, B, band)
    full = (bandf * benv).numpy()
    rows = pr.kept_ky(H, g.kyp, g.kyn)
    got = full[rows][:, :g.nkx].T
    assert np.array_equal(got != 0, kept), "band decisions differ from the oracle's"
    outside = full.copy()
    outside[rows[:, None], np.arange(g.nkx)[None, :]] = 0
    assert not outside.any()
    err = np.abs(got.astype(np.float64) - value)
    assert (err[~kept] == 0).all() and kept.any()
    print(f"RATIO xc filter {what}: oracle {(err[kept] / bound[kept]).max():.3f}")
    assert (err[kept] < bound[kept]).all()
    if B == 0:
        assert (value[kept] == 1).all() and (bound[kept] == 2 * U).all()


def test_filter_cases_reach_their_edges():
    by = {c[5]: c for c in pr.FILTER_CASES}
    g, low, high = filter_args(by["band edges on bins"])
    assert (low, high) == (0.125, 0.25)
    kept, _, _ = pr.filter64(64, 64, g.nkx, g.kyp, g.kyn, low, high, 500.0, 1.0)
    rows = pr.kept_ky(64, g.kyp, g.kyn).tolist()
    assert kept[0, rows.index(16)] and kept[16, 0] and kept[0, rows.index(48)]    # f == high: included
    assert not kept[0, rows.index(8)] and not kept[8, 0] and kept[0, rows.index(9)]  # f == low: excluded
    g, _, _ = filter_args(by["kyn = 0"])
    assert (g.kyp, g.kyn) == (32, 0)   # high = 0.5 keeps every row: xc_geometry reports them all as kyp
    g, low, high = filter_args(by["odd H, every row kept"])
    kept, _, _ = pr.filter64(64, 63, g.nkx, g.kyp, g.kyn, low, high, 500.0, 1.0)
    assert (g.kyp, g.kyn) == (63, 0) and kept[0, 31] and kept[0, 32]   # rows +31 and -31: 31 / 63 <= 0.5 < 32 / 63
    assert sum(c[0] % 2 for c in pr.FILTER_CASES) >= 3 and sum(c[0] != c[1] for c in pr.FILTER_CASES) >= 4
    g, low, high = filter_args(by["odd H"])
    kept, _, _ = pr.filter64(64, 63, g.nkx, g.kyp, g.kyn, low, high, 500.0, 1.0)
    assert g.kyn >= 1 and kept[:, g.kyp:].any()  # negative rows are kept: the sign rule matters


# ------------------------------------------------------------------ argument rules (no launch)


def test_entry_points_reject_bad_arguments_before_any_launch():
    lib = _lib.load()
    a, b = ctypes.c_void_p(16), ctypes.c_void_p(4096)  # non-null addresses: argument checks never dereference them
    bad = -1  # MC_ERR_ARG
    assert lib.mc_field_smooth_center(a, b, 5, 6, 6, 0, None) == bad      # window > t
    assert lib.mc_field_smooth_center(a, a, 5, 6, 3, 1, None) == bad      # in place with window >= 3
    assert lib.mc_field_smooth_center(a, b, 0, 6, 0, 0, None) == bad and lib.mc_field_smooth_center(a, b, 5, 0, 0, 0, None) == bad
    assert lib.mc_field_smooth_center(None, b, 5, 6, 0, 0, None) == bad and lib.mc_field_smooth_center(a, None, 5, 6, 0, 0, None) == bad
    assert lib.mc_xc_ref_mean_except_current(a, a, a, a, a, b, 1, 3, 10, 1.0, None) == bad   # t < 2
    assert lib.mc_xc_ref_mean_except_current(a, a, a, a, a, b, 4, 0, 10, 1.0, None) == bad
    assert lib.mc_xc_ref_mean_except_current(a, a, a, a, a, b, 4, 3, 0, 1.0, None) == bad
    assert lib.mc_xc_ref_mean_except_current(a, a, a, a, None, b, 4, 3, 10, 1.0, None) == bad
    assert lib.mc_circle_mask(a, b, 16, 16, -1.0, 2.0, None) == bad and lib.mc_circle_mask(a, b, 16, 16, 4.0, float("nan"), None) == bad
    assert lib.mc_circle_mask(a, b, 0, 16, 4.0, 2.0, None) == bad and lib.mc_circle_mask(a, None, 16, 16, 4.0, 2.0, None) == bad
    g = plan.xc_geometry(64, 64, 0.1, 16, 8)
    assert lib.mc_xc_filter(a, g, 0.0, 0.1, 500.0, 0.0, None) == bad and lib.mc_xc_filter(None, g, 0.0, 0.1, 500.0, 1.0, None) == bad
    empty = _lib.XcGeom(W=64, H=64, nkx=0, kyp=4, kyn=3, y0=0, ny=64, x0=0, x1=64, RG=16)
    assert lib.mc_xc_filter(a, empty, 0.0, 0.1, 500.0, 1.0, None) == bad
    assert lib.mc_spline_lattice(a, 0, 2, 2, 2, a, a, 3, a, a, 3, a, a, 3, b, None) == bad
    assert lib.mc_spline_lattice(a, 2, 2, 2, 2, a, a, 3, a, a, 0, a, a, 3, b, None) == bad
    assert lib.mc_spline_lattice(a, 2, 2, 2, 2, a, None, 3, a, a, 3, a, a, 3, b, None) == bad
    assert lib.mc_spline_points(a, 2, 2, 2, 2, a, a, a, a, a, a, 0, b, None) == bad
    assert lib.mc_spline_points(a, 2, 2, 0, 2, a, a, a, a, a, a, 5, b, None) == bad
