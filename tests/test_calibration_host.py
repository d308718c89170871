"""Gain-reference and defect-map estimation, without a GPU: the names exist, the header and the ctypes table agree
on the new entry point, arguments are checked before any device is touched, and the integer / float64 rules -- as
tests/calibration_reference.py restates them and as the package evaluates them on saved accumulators -- give the
hand-worked answers on 4 x 4 cases."""

import ctypes
import inspect

import numpy as np
import pytest
import torch

import calibration_reference as cr
from kernel_harness import assert_entry_point
import torch_motion_correction_amd as mc
from torch_motion_correction_amd import _lib, calibration


def test_names_exist():
    for name in ("RawStatistics", "estimate_defect_map", "estimate_gain_reference"):
        assert name in mc.__all__ and getattr(mc, name) is getattr(calibration, name)
    assert list(inspect.signature(mc.RawStatistics).parameters) == ["shape", "device"]
    sig = inspect.signature(mc.estimate_defect_map)
    assert list(sig.parameters) == ["stats", "hot_factor", "dead_factor"]
    assert sig.parameters["hot_factor"].default == 5.0 and sig.parameters["dead_factor"].default == 0.2
    sig = inspect.signature(mc.estimate_gain_reference)
    assert list(sig.parameters) == ["stats_or_movies", "defect_map", "return_defect_map"]
    assert sig.parameters["defect_map"].default is None and sig.parameters["return_defect_map"].default is False
    for name in ("add", "merge", "from_sums"):
        assert callable(getattr(mc.RawStatistics, name))


def test_header_and_signatures_agree_on_the_new_entry_point():
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    assert_entry_point("mc_raw_pixel_sums", [vp, i32, i32, i32, i32, vp, vp, vp])


def test_entry_point_validates_on_the_host():
    """Fake pointers and a null stream: every call below must answer MC_ERR_ARG before it launches anything."""
    lib = _lib.load()
    p = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(3)]

    def call(raw=p[0], is_i16=0, t=4, h=8, w=8, s=p[1], q=p[2]):
        return lib.mc_raw_pixel_sums(raw, is_i16, t, h, w, s, q, None)

    for name in ("raw", "s", "q"):
        assert call(**{name: None}) == -1, name
    assert call(t=0) == -1 and call(h=0) == -1 and call(w=0) == -1 and call(t=-3) == -1
    assert call(is_i16=2) == -1 and call(is_i16=-1) == -1
    assert call(raw=ctypes.c_void_p(0x100001), is_i16=1) == -1  # an i16 movie at an odd address
    assert call(s=ctypes.c_void_p(0x200004)) == -1 and call(q=ctypes.c_void_p(0x300004)) == -1
    assert call(h=1 << 30, w=1 << 30) == -1  # more pieces than a grid holds


# ------------------------------------------------------------------ argument rules, devices refused


def _refuse_devices(monkeypatch):
    from torch_motion_correction_amd import api

    def refuse(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    for module in (api, calibration):
        monkeypatch.setattr(module, "require_gpu", refuse)
        monkeypatch.setattr(module, "device_scope", refuse)


def _saved(sum_, sumsq, n, dtype=torch.uint8):
    return mc.RawStatistics.from_sums(torch.as_tensor(np.asarray(sum_, dtype=np.int64)),
                                      torch.as_tensor(np.asarray(sumsq, dtype=np.int64)), n, dtype)


def test_argument_rules_hold_before_any_device_is_touched(monkeypatch):
    _refuse_devices(monkeypatch)
    for bad in ((4,), (4, 4, 4), (0, 4), "ab", None):
        with pytest.raises(ValueError, match="shape must be"):
            mc.RawStatistics(bad)
    st = mc.RawStatistics((4, 6))
    assert st.frames == 0 and st.sum is None and st.sumsq is None and st.dtype is None
    for movie in (torch.zeros(2, 4, 6), torch.zeros(2, 4, 6, dtype=torch.float16), torch.zeros(2, 4, 6).long(),
                  np.zeros((2, 4, 6), dtype=np.uint8)):
        with pytest.raises(ValueError, match="uint8 or int16"):  # a float (or any other) movie
            st.add(movie)
    for movie in (torch.zeros(6, dtype=torch.uint8), torch.zeros(1, 2, 4, 6, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\(t, h, w\) or \(h, w\)"):  # wrong rank
            st.add(movie)
    for movie in (torch.zeros(2, 6, 4, dtype=torch.uint8), torch.zeros(4, 5, dtype=torch.int16)):
        with pytest.raises(ValueError, match="these statistics are for"):  # not the frame size of `shape`
            st.add(movie)
    with pytest.raises(ValueError, match="at least one frame"):
        st.add(torch.zeros(0, 4, 6, dtype=torch.uint8))
    held = _saved(np.ones((4, 6)), np.ones((4, 6)), 3)
    with pytest.raises(ValueError, match="cannot be mixed"):  # mixed dtypes
        held.add(torch.zeros(1, 4, 6, dtype=torch.int16))
    with pytest.raises(ValueError, match="cannot be mixed"):
        held.merge(_saved(np.ones((4, 6)), np.ones((4, 6)), 3, torch.int16))
    with pytest.raises(ValueError, match="merge takes"):
        held.merge(_saved(np.ones((4, 4)), np.ones((4, 4)), 3))
    # empty statistics
    for fn in (mc.estimate_defect_map, mc.estimate_gain_reference):
        with pytest.raises(ValueError, match="no frames were added"):
            fn(st)
    with pytest.raises(ValueError, match="no frames were added"):
        mc.estimate_gain_reference([])
    with pytest.raises(ValueError, match="RawStatistics"):
        mc.estimate_defect_map(torch.zeros(4, 6))
    for kw in (dict(hot_factor=0.1), dict(dead_factor=6.0), dict(hot_factor=float("nan"))):
        with pytest.raises(ValueError, match="dead_factor < hot_factor"):
            mc.estimate_defect_map(held, **kw)
    with pytest.raises(ValueError, match="defect_map must be"):
        mc.estimate_gain_reference(held, defect_map=torch.zeros(4, 6))
    assert st.frames == 0 and st.sum is None and held.frames == 3


def test_frames_are_refused_before_sumsq_can_overflow(monkeypatch):
    """sumsq is int64: 255^2 n (u8) and 2^30 n (i16) pass 2^63 - 1 beyond MAX_FRAMES."""
    _refuse_devices(monkeypatch)
    assert calibration.MAX_FRAMES == {torch.uint8: (2**63 - 1) // 255**2, torch.int16: 2**33 - 1}
    for dtype, worst in ((torch.uint8, 255**2), (torch.int16, 2**30)):
        top = calibration.MAX_FRAMES[dtype]
        assert worst * top <= 2**63 - 1 < worst * (top + 1)
        full = _saved(np.ones((2, 2)), np.ones((2, 2)), top, dtype)
        with pytest.raises(ValueError, match="could overflow"):
            full.add(torch.zeros(1, 2, 2, dtype=dtype))
        with pytest.raises(ValueError, match="could overflow"):
            _saved(np.ones((2, 2)), np.ones((2, 2)), 1, dtype).merge(full)
        with pytest.raises(ValueError, match="frames must be"):
            _saved(np.ones((2, 2)), np.ones((2, 2)), top + 1, dtype)


# ------------------------------------------------------------------ the rules on hand-made 4 x 4 cases


def hand_made_movie():
    """n = 4 frames of 4 x 4 u8.  Pixel sums: (0,0) dead, 0; (1,1) 80 = exactly 5 x the mean sum; (2,2) stuck at 3,
    sum 12; eight pixels of sum 13 and five of sum 12 that vary.  Total 256 = 16 pixels x 16: n M = 16.0 exactly, so
    the thresholds 0.2 * 4 * 4.0 = 3.2 (rounded) and 5.0 * 4 * 4.0 = 80.0 (exact) are what the comparisons see."""
    m = np.zeros((4, 4, 4), dtype=np.uint8)
    m[:] = np.array([3, 3, 4, 3], dtype=np.uint8)[:, None, None]  # sum 13
    for y, x in ((0, 1), (0, 2), (0, 3), (3, 0), (3, 1)):
        m[:, y, x] = [2, 3, 4, 3]  # sum 12, not constant
    m[:, 0, 0] = 0
    m[:, 1, 1] = [20, 20, 19, 21]
    m[:, 2, 2] = 3
    return m


def both(sum_, sumsq, n, dtype=torch.uint8, **kw):
    """The defect map of the restatement, after checking that the package gives the same on saved accumulators."""
    want = cr.defect_map(sum_, sumsq, n, **kw)
    got = mc.estimate_defect_map(_saved(sum_, sumsq, n, dtype), **kw)
    assert got.dtype == torch.bool and np.array_equal(got.numpy(), want)
    return want


def test_defect_rules_on_a_hand_made_case():
    m = hand_made_movie()
    s, q = cr.pixel_sums(m)
    assert int(s.sum()) == 256 and s[1, 1] == 80 and s[2, 2] == 12 and q[2, 2] == 36
    d = both(s, q, 4)
    planted = np.zeros((4, 4), dtype=bool)
    planted[0, 0] = planted[1, 1] = planted[2, 2] = True
    assert np.array_equal(d, planted)
    # each rule alone: >= at exactly 5 x M, and not beyond it
    assert np.array_equal(both(s, q, 4, hot_factor=5.000001), planted & (s != 80))
    assert np.array_equal(both(s, q, 4, dead_factor=0.0), planted)  # sum 0 <= 0 is still dead
    assert not both(s, q, 4, hot_factor=5.000001, dead_factor=0.0)[1, 1]
    # one more count in one frame and the stuck pixel is an ordinary one
    m2 = m.copy()
    m2[3, 2, 2] = 4
    s2, q2 = cr.pixel_sums(m2)
    assert not both(s2, q2, 4)[2, 2]


def test_one_frame_switches_the_stuck_rule_off():
    """n = 1: n * sumsq == sum^2 for every pixel, which says nothing."""
    m = hand_made_movie()[:1]
    s, q = cr.pixel_sums(m)
    assert np.array_equal(q, s * s)
    d = both(s, q, 1)
    assert d[0, 0] and int(d.sum()) == 2 and d[1, 1]  # the dead pixel, and 20 >= 5 * 57 / 16
    assert not d[2, 2]


def test_stuck_rule_is_exact_for_negative_values_and_beyond_int64_squares():
    n = 4
    s = np.full((4, 4), 40, dtype=np.int64)
    q = np.full((4, 4), 402, dtype=np.int64)  # 10, 10, 9, 11
    s[0, 0], q[0, 0] = -20, 100  # -5 in every frame
    s[0, 1], q[0, 1] = -21, 111  # -5, -5, -5, -6: n does not divide the sum
    s[0, 2], q[0, 2] = -20, 102  # -5, -5, -4, -6: the sum of a stuck pixel, not its squares
    d = both(s, q, n, dtype=torch.int16, hot_factor=1e9, dead_factor=-1e9)  # the stuck rule alone
    assert d[0, 0] and int(d.sum()) == 1
    # 100 000 i16 frames stuck at -32768: sum^2 = 1.07e19 > 2^63, the rule still holds in both evaluations
    n = 100_000
    s = np.full((4, 4), 7 * n + 1, dtype=np.int64)
    q = np.full((4, 4), 49 * n + 15, dtype=np.int64)
    s[3, 3], q[3, 3] = -32768 * n, 2**30 * n
    s[3, 2], q[3, 2] = 32767 * n, 32767**2 * n
    s[3, 1], q[3, 1] = 32767 * n, 32767**2 * n + 2  # one frame up, one down
    assert int(s[3, 3]) ** 2 > 2**63
    d = both(s, q, n, dtype=torch.int16, hot_factor=1e9, dead_factor=-1e9)
    assert d[3, 3] and d[3, 2] and int(d.sum()) == 2


def test_gain_rule_on_the_hand_made_case():
    m = hand_made_movie()
    s, q = cr.pixel_sums(m)
    d = cr.defect_map(s, q, 4)
    want = cr.gain_reference(s, d)
    assert want.dtype == np.float32 and not want[d].any()
    # T = 164 over c = 13 good pixels: one Python division of exact integers is the correctly rounded quotient
    assert want[0, 1] == np.float32(164 / (13 * 12)) and want[1, 0] == np.float32(164 / (13 * 13))
    st = _saved(s, q, 4)
    gain, dmap = mc.estimate_gain_reference(st, return_defect_map=True)
    assert gain.dtype == torch.float32 and np.array_equal(gain.numpy(), want) and np.array_equal(dmap.numpy(), d)
    assert torch.equal(mc.estimate_gain_reference(st), gain)
    # a caller's own map replaces the estimated one
    own = torch.zeros(4, 4, dtype=torch.bool)
    own[0, 0] = True
    assert np.array_equal(mc.estimate_gain_reference(st, defect_map=own).numpy(), cr.gain_reference(s, own.numpy()))


def test_gain_refuses_what_has_no_multiplicative_gain():
    ones = np.ones((4, 4), dtype=np.int64)
    with pytest.raises(ValueError, match="no pixel is good"):
        mc.estimate_gain_reference(_saved(8 * ones, 40 * ones, 2), defect_map=torch.ones(4, 4, dtype=torch.bool))
    with pytest.raises(ValueError, match="no pixel is good"):
        mc.estimate_gain_reference(_saved(8 * ones, 32 * ones, 2))  # every pixel stuck at 4
    neg = -8 * ones
    neg[0, 0] = 3
    none = torch.zeros(4, 4, dtype=torch.bool)
    with pytest.raises(ValueError, match="must be positive"):  # i16 and T <= 0
        mc.estimate_gain_reference(_saved(neg, 40 * ones, 2, torch.int16), defect_map=none)
    with pytest.raises(ValueError, match="must be positive"):  # a good pixel that never counted
        zero = 8 * ones
        zero[1, 1] = 0
        mc.estimate_gain_reference(_saved(zero, 40 * ones, 2), defect_map=none)
    with pytest.raises(ValueError, match="2\\^53"):
        mc.estimate_gain_reference(_saved(2**50 * ones, 2**51 * ones, 2**40), defect_map=none)


def test_merge_adds_the_accumulators():
    m = hand_made_movie()
    sa, qa = cr.pixel_sums(m[:1])
    sb, qb = cr.pixel_sums(m[1:])
    a, b = _saved(sa, qa, 1), _saved(sb, qb, 3)
    empty = mc.RawStatistics((4, 4))
    assert empty.merge(a) is empty and empty.frames == 1 and empty.dtype == torch.uint8
    empty.merge(b).merge(mc.RawStatistics((4, 4)))
    s, q = cr.pixel_sums(m)
    assert empty.frames == 4 and np.array_equal(empty.sum.numpy(), s) and np.array_equal(empty.sumsq.numpy(), q)
    assert np.array_equal(a.sum.numpy(), sa) and a.frames == 1  # the merged-in instance is left as it was
