"""The detector-defect fill (DefectFill, fill_defects_raw, fill_defects_gain, defect_map_from_rectangles), without a
GPU: names and parameter lists, the header, the ctypes table and the build list on the three entry points, every
argument rule before any device is touched, the entry points' host checks with fake pointers, the rectangles, the
rule's restatement (tests/defect_reference.py) on hand-made cases, the pick's uniformity on the restatement, and the
kernels' per-thread bodies run thread by thread on the CPU under the address and undefined-behaviour sanitizers
(tests/host_defect_fill.cpp, a stand-alone program started as a child process)."""

import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import defect_reference as dr
from kernel_harness import assert_entry_point, header_parameters, run_host_program
import torch_motion_correction_amd as mc
from torch_motion_correction_amd import _lib, calibration

ENTRIES = {"mc_defect_donors": 9, "mc_raw_fill_defects": 12, "mc_gain_fill_defects": 9}
ARG = -1


# ------------------------------------------------------------------ exports


def test_names_and_parameter_lists():
    for name in ("DefectFill", "fill_defects_raw", "fill_defects_gain", "defect_map_from_rectangles"):
        assert name in mc.__all__ and getattr(mc, name) is getattr(calibration, name)
    sig = inspect.signature(mc.DefectFill)
    assert list(sig.parameters) == ["defect_map", "reach", "device"]
    assert sig.parameters["reach"].default == 4 and sig.parameters["device"].default is None
    sig = inspect.signature(mc.fill_defects_raw)
    assert list(sig.parameters) == ["movie", "fill", "seed", "in_place", "device"]
    assert (sig.parameters["seed"].default, sig.parameters["in_place"].default, sig.parameters["device"].default) == \
        (0, False, None)
    sig = inspect.signature(mc.fill_defects_gain)
    assert list(sig.parameters) == ["gain", "fill", "device"] and sig.parameters["device"].default is None
    assert list(inspect.signature(mc.defect_map_from_rectangles).parameters) == ["shape", "rectangles"]


def test_header_signatures_and_build_list_agree_on_the_entry_points():
    from torch_motion_correction_amd import _build

    for name, count in ENTRIES.items():
        assert_entry_point(name, source=("defect_fill.hip", "defect_fill", []))
        assert len(header_parameters(name)) == len(_lib.SIGNATURES[name]) == count, name
    assert _lib.SIGNATURES["mc_raw_fill_defects"][10] is ctypes.c_uint  # the seed
    assert os.path.exists(os.path.join(_build.CSRC, "defect_fill.h"))


# ------------------------------------------------------------------ the C entry points' host checks


def _calls():
    """call(entry, **changed arguments) with fake pointers and a null stream: every answer comes before a launch."""
    lib = _lib.load()
    p = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(4)]
    base = dict(data=p[0], es=2, t=3, h=8, w=16, pixels=p[1], n=5, reach=4, donors=p[2], counts=p[3], seed=0)

    def call(entry, **kw):
        a = dict(base, **kw)
        if entry == "mc_defect_donors":
            return lib.mc_defect_donors(a["data"], a["h"], a["w"], a["pixels"], a["n"], a["reach"], a["donors"],
                                        a["counts"], None)
        if entry == "mc_raw_fill_defects":
            return lib.mc_raw_fill_defects(a["data"], a["es"], a["t"], a["h"], a["w"], a["pixels"], a["donors"],
                                           a["counts"], a["n"], a["reach"], a["seed"], None)
        return lib.mc_gain_fill_defects(a["data"], a["h"], a["w"], a["pixels"], a["donors"], a["counts"], a["n"],
                                        a["reach"], None)

    return call


def test_entry_points_refuse_null_pointers():
    call = _calls()
    for entry in ENTRIES:
        for name in ("data", "pixels", "donors", "counts"):
            assert call(entry, **{name: None}) == ARG, (entry, name)
        assert call(entry, data=None, n=0) == ARG, entry  # the map, the movie and the gain even without defects


def test_entry_points_refuse_bad_ranges():
    call = _calls()
    for entry in ENTRIES:
        for reach in (0, -1, 17, 1 << 20):
            assert call(entry, reach=reach) == ARG, (entry, reach)
            assert call(entry, reach=reach, n=0) == ARG, (entry, reach)
        for kw in (dict(h=0), dict(w=0), dict(h=-8), dict(n=-1), dict(n=8 * 16 + 1), dict(h=1 << 16, w=1 << 15)):
            assert call(entry, **kw) == ARG, (entry, kw)  # the last: 2^31 pixels, beyond an int index
    for es in (0, 3, 8, -1, 16):
        assert call("mc_raw_fill_defects", es=es) == ARG, es
    assert call("mc_raw_fill_defects", t=0) == ARG and call("mc_raw_fill_defects", t=-4) == ARG
    odd = ctypes.c_void_p(0x100001)
    assert call("mc_raw_fill_defects", data=odd, es=2) == ARG and call("mc_raw_fill_defects", data=odd, es=4) == ARG
    assert call("mc_raw_fill_defects", data=ctypes.c_void_p(0x100002), es=4) == ARG
    assert call("mc_gain_fill_defects", data=ctypes.c_void_p(0x100002)) == ARG


def test_entry_points_answer_zero_defects_without_a_launch():
    call = _calls()
    for entry in ENTRIES:
        assert call(entry, n=0) == 0, entry
        assert call(entry, n=0, pixels=None, donors=None, counts=None) == 0, entry  # empty tensors have no address
        assert call(entry, n=0, reach=1) == 0 and call(entry, n=0, reach=16) == 0, entry
    for es in (1, 2, 4):
        assert call("mc_raw_fill_defects", n=0, es=es) == 0
    assert call("mc_raw_fill_defects", n=0, data=ctypes.c_void_p(0x100001), es=1) == 0


# ------------------------------------------------------------------ argument rules, devices refused


def _refuse_devices(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    monkeypatch.setattr(calibration, "require_gpu", refuse)
    monkeypatch.setattr(calibration, "device_scope", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def test_argument_rules_hold_before_any_device_is_touched(monkeypatch):
    _refuse_devices(monkeypatch)
    dmap = torch.zeros(8, 16, dtype=torch.bool)
    dmap[3, 5] = True
    u8 = torch.zeros(4, 8, 16, dtype=torch.uint8)
    gain = torch.ones(8, 16)
    # the map
    for bad in (torch.zeros(8, 16), torch.zeros(8, 16, dtype=torch.uint8), torch.zeros(16, dtype=torch.bool),
                torch.zeros(2, 8, 16, dtype=torch.bool), torch.zeros(0, 16, dtype=torch.bool),
                np.zeros((8, 16), dtype=bool), None):
        with pytest.raises(ValueError, match=r"bool \(h, w\) tensor"):
            mc.DefectFill(bad)
        with pytest.raises(ValueError, match=r"bool \(h, w\) tensor"):
            mc.fill_defects_raw(u8, bad)
        with pytest.raises(ValueError, match=r"bool \(h, w\) tensor"):
            mc.fill_defects_gain(gain, bad)
    for reach in (0, -1, 17, 4.0, None, True, "4"):
        with pytest.raises(ValueError, match=r"reach must be an int in 1\.\.16"):
            mc.DefectFill(dmap, reach)
    # the movie
    for movie in (torch.zeros(4, 8, 16, dtype=torch.int32), torch.zeros(4, 8, 16, dtype=torch.float64),
                  torch.zeros(4, 8, 16, dtype=torch.int8), torch.zeros(4, 8, 16, dtype=torch.bfloat16),
                  torch.zeros(4, 8, 16, dtype=torch.bool), np.zeros((4, 8, 16), dtype=np.uint8)):
        with pytest.raises(ValueError, match="uint8, int16, float16 or float32"):
            mc.fill_defects_raw(movie, dmap)
    for movie in (torch.zeros(16, dtype=torch.uint8), torch.zeros(1, 4, 8, 16, dtype=torch.uint8),
                  torch.zeros(0, 8, 16, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\(t, h, w\) or \(h, w\)"):
            mc.fill_defects_raw(movie, dmap)
    for dtype in (torch.uint8, torch.int16, torch.float16, torch.float32):
        for shape in ((4, 16, 8), (4, 8, 15), (9, 16), (4, 7, 16)):
            with pytest.raises(ValueError, match="the defect map has shape"):
                mc.fill_defects_raw(torch.zeros(shape, dtype=dtype), dmap)
    for seed in (-1, 2**32, 1.0, None, True, "0"):
        with pytest.raises(ValueError, match="seed must be an int in 0"):
            mc.fill_defects_raw(u8, dmap, seed=seed)
    with pytest.raises(ValueError, match="in_place=True needs a contiguous movie that is already on the GPU"):
        mc.fill_defects_raw(u8, dmap, in_place=True)  # a CPU movie
    # the gain
    for bad in (torch.ones(8, 16, dtype=torch.float64), torch.ones(8, 16, dtype=torch.float16), torch.ones(2, 8, 16),
                torch.ones(16), np.ones((8, 16), dtype=np.float32)):
        with pytest.raises(ValueError, match=r"gain must be a float32 \(h, w\) tensor"):
            mc.fill_defects_gain(bad, dmap)
    for bad in (torch.ones(16, 8), torch.ones(8, 15)):
        with pytest.raises(ValueError, match="the defect map has shape"):
            mc.fill_defects_gain(bad, dmap)


# ------------------------------------------------------------------ MotionCor2 defect-file rectangles


def test_rectangles():
    got = mc.defect_map_from_rectangles((6, 10), [(2, 1, 3, 2)])  # x 2..4, y 1..2
    want = np.zeros((6, 10), dtype=bool)
    want[1:3, 2:5] = True
    assert got.dtype == torch.bool and got.device.type == "cpu" and np.array_equal(got.numpy(), want)
    assert not mc.defect_map_from_rectangles((6, 10), []).any()
    # a dead column, a dead row, rectangles that touch the right and the bottom edge, an overlap, the whole frame
    got = mc.defect_map_from_rectangles((6, 10), [(7, 0, 1, 6), (0, 5, 10, 1), (8, 3, 2, 3), [0, 0, 1, 1],
                                                  np.array([7, 2, 2, 2])])
    want = np.zeros((6, 10), dtype=bool)
    want[:, 7] = want[5, :] = want[0, 0] = True
    want[3:6, 8:10] = want[2:4, 7:9] = True
    assert np.array_equal(got.numpy(), want)
    assert bool(mc.defect_map_from_rectangles((6, 10), [(0, 0, 10, 6)]).all())
    # one pixel across an edge, on each side
    for rect in ((8, 3, 3, 3), (8, 3, 2, 4), (-1, 0, 2, 2), (0, -1, 2, 2), (10, 0, 1, 1), (0, 6, 1, 1), (0, 0, 11, 1)):
        with pytest.raises(ValueError, match="leaves the"):
            mc.defect_map_from_rectangles((6, 10), [(1, 1, 1, 1), rect])
    for rect in ((1, 1, 0, 2), (1, 1, 2, 0), (1, 1, -2, 2), (20, 20, 0, 0)):
        with pytest.raises(ValueError, match="is empty"):
            mc.defect_map_from_rectangles((6, 10), [rect])
    for rect in ((1.0, 1, 2, 2), (1, 1, 2.5, 2), ("1", 1, 2, 2), (1, 1, 2), (1, 1, 2, 2, 2), 7, None,
                 (1, 1, True, 2), (1, float("nan"), 2, 2)):
        with pytest.raises(ValueError, match="must be four integers"):
            mc.defect_map_from_rectangles((6, 10), [rect])
    for shape in ((6,), (0, 10), (6, 10, 2), (6.0, 10), None):
        with pytest.raises(ValueError, match="shape must be"):
            mc.defect_map_from_rectangles(shape, [])


# ------------------------------------------------------------------ the restatement, by hand


def _single(h, w, y, x):
    m = np.zeros((h, w), dtype=bool)
    m[y, x] = True
    return m


def test_donor_rule_on_hand_made_cases():
    h, w = 7, 9
    # corner: 3, edge: 5, interior: 8 -- in row-major order
    pixels, donors, counts = dr.donor_table(_single(h, w, 0, 0), 4)
    assert pixels.tolist() == [0] and counts.tolist() == [3] and donors.shape == (1, 32)
    assert donors[0, :3].tolist() == [1, w, w + 1] and (donors[0, 3:] == -1).all()
    pixels, donors, counts = dr.donor_table(_single(h, w, h - 1, w - 1), 1)
    assert counts.tolist() == [3] and donors.shape == (1, 8)
    assert donors[0, :3].tolist() == [(h - 2) * w + w - 2, (h - 2) * w + w - 1, (h - 1) * w + w - 2]
    pixels, donors, counts = dr.donor_table(_single(h, w, 0, 4), 4)
    assert counts.tolist() == [5] and donors[0, :5].tolist() == [3, 5, w + 3, w + 4, w + 5]
    pixels, donors, counts = dr.donor_table(_single(h, w, 3, 4), 4)
    p = 3 * w + 4
    assert pixels.tolist() == [p] and counts.tolist() == [8]
    assert donors[0, :8].tolist() == [p - w - 1, p - w, p - w + 1, p - 1, p + 1, p + w - 1, p + w, p + w + 1]
    # a full dead column: an interior pixel has the 6 off-column pixels of ring 1, its ends 4
    col = np.zeros((h, w), dtype=bool)
    col[:, 4] = True
    pixels, donors, counts = dr.donor_table(col, 4)
    assert pixels.tolist() == [y * w + 4 for y in range(h)] and counts.tolist() == [4, 6, 6, 6, 6, 6, 4]
    assert donors[3, :6].tolist() == [2 * w + 3, 2 * w + 5, 3 * w + 3, 3 * w + 5, 4 * w + 3, 4 * w + 5]
    assert donors[0, :4].tolist() == [3, 5, w + 3, w + 5] and (donors[0, 4:] == -1).all()
    # a 3 x 3 block: the centre's ring 1 is all defects, its ring 2 all good (16 donors); reach 1 finds none
    block = np.zeros((h, w), dtype=bool)
    block[2:5, 3:6] = True
    pixels, donors, counts = dr.donor_table(block, 2)
    centre = pixels.tolist().index(3 * w + 4)
    assert counts[centre] == 16 and donors.shape[1] == 16 and (donors[centre] >= 0).all()
    assert len(dr.ring(3, 4, 2, h, w)) == 16 and donors[centre, 0] == 1 * w + 2 and donors[centre, -1] == 5 * w + 6
    assert dr.donor_table(block, 1)[2][centre] == 0 and dr.first_without_donor(block, 1) == (3, 4)
    assert dr.first_without_donor(block, 2) is None
    # no defects
    pixels, donors, counts = dr.donor_table(np.zeros((h, w), dtype=bool), 4)
    assert pixels.shape == (0,) and donors.shape == (0, 32) and counts.shape == (0,)


def test_fill_rule_on_hand_made_cases():
    # the pick in Python integers: hand-checked corner values of the rule
    assert dr.pick(0, 0, 0, 8) == 0  # x = 0 stays 0 through the finaliser
    for seed, f, j, c in ((1, 0, 0, 8), (0, 39, 23456, 24), (2**32 - 1, 65535, 2**31 - 1, 128)):
        k = dr.pick(seed, f, j, c)
        assert 0 <= k < c and k == int(dr.picks(seed, f, j, c))
    rs = np.random.RandomState(0)
    for _ in range(2000):  # the array form is the integer form
        seed, f, j, c = int(rs.randint(0, 2**32, dtype=np.uint64)), int(rs.randint(0, 70000)), \
            int(rs.randint(0, 2**31)), int(rs.randint(1, 129))
        assert dr.pick(seed, f, j, c) == int(dr.picks(seed, f, j, c))
    # a dead column in a movie whose value is its own linear index: the filled value names the donor
    t, h, w = 6, 5, 8
    col = np.zeros((h, w), dtype=bool)
    col[:, 3] = True
    movie = np.arange(t * h * w, dtype=np.int16).reshape(t, h, w)
    out = dr.fill(movie, col, 4, 12345)
    assert out.dtype == np.int16 and np.array_equal(out[:, ~col], movie[:, ~col])
    pixels, donors, counts = dr.donor_table(col, 4)
    for f in range(t):
        for j, p in enumerate(pixels):
            d = int(out[f].reshape(-1)[p]) - f * h * w
            assert d == donors[j, dr.pick(12345, f, j, int(counts[j]))] and d in donors[j, :counts[j]].tolist()
    assert not np.array_equal(out, dr.fill(movie, col, 4, 0))  # the seed matters
    assert np.array_equal(dr.fill(movie[0], col, 4, 7), dr.fill(movie[:1], col, 4, 7)[0])  # (h, w) is one frame
    # bits travel: a NaN payload in a donor arrives as it is
    f32 = np.ones((1, 1, 2), dtype=np.float32)
    f32.view(np.uint32)[0, 0, 1] = 0x7FC12345
    got = dr.fill(f32, np.array([[True, False]]), 1, 0)
    assert got.view(np.uint32).tolist() == [[[0x7FC12345, 0x7FC12345]]]
    # the gain: the float64 mean of the donors in table order, rounded once
    gain = np.zeros((h, w), dtype=np.float32)
    gain[~col] = (1.0 + np.arange(h * w - h, dtype=np.float32) / 3).astype(np.float32)
    filled = dr.gain_fill(gain, col, 4)
    assert filled.dtype == np.float32 and np.array_equal(filled[~col], gain[~col]) and (filled[col] > 0).all()
    j = 2  # (2, 3)
    want = np.float32(sum(float(gain.reshape(-1)[d]) for d in donors[j, :6]) / 6)
    assert filled[2, 3] == want
    with pytest.raises(AssertionError, match="no donor"):
        dr.fill(movie, np.ones((h, w), dtype=bool), 4, 0)


# ------------------------------------------------------------------ the pick is uniform


def test_hash_uniformity():
    """8192 picks over f at fixed j, and over j at fixed f: every bin within 5 binomial standard deviations of
    8192 / count.  A condition on the rule (the restatement only; the kernels are pinned to the restatement)."""
    n = 8192
    run = np.arange(n)
    worst = 0.0
    for seed in (0, 1, 12345):
        for count in (1, 2, 3, 5, 6, 8, 24, 32):
            sd = (n * (1 / count) * (1 - 1 / count)) ** 0.5
            series = [dr.picks(seed, run, j, count) for j in (0, 1, 7, 1000, 23456)]
            series += [dr.picks(seed, f, run, count) for f in (0, 1, 39)]
            for k in series:
                bins = np.bincount(k, minlength=count)
                assert len(bins) == count and int(bins.sum()) == n
                dev = float(np.abs(bins - n / count).max())
                assert dev <= 5 * sd, (seed, count, bins.tolist())
                worst = max(worst, dev / sd if sd else 0.0)
    print(f"worst bin: {worst:.2f} standard deviations")


# ------------------------------------------------------------------ the kernels' bodies on the CPU, sanitized


def test_kernel_bodies_on_the_host_under_sanitizers(tmp_path):
    """csrc/defect_fill.h -- the per-thread bodies defect_fill.hip compiles for the device -- is built for the host
    with -fsanitize=address,undefined into a program of its own and run as a child process: every thread of
    defect_donors, raw_fill_defects<1, 2, 4> and gain_fill_defects in turn on exactly-sized heap buffers, at the
    frames, reaches and seeds of tests/test_defect_fill.py, a view one element into its allocation, a map with a
    defect that has no donor, a map without defects and a map without good pixels, against naive loops, and tables
    that cannot be used (counts and indices out of range), which must leave the movie and the gain untouched.  Nothing
    sanitized is loaded into this process.  Needs clang++; the ROCm one is used."""
    res = run_host_program("host_defect_fill.cpp", tmp_path)
    assert res.stdout.count(": ok") == 136
