"""MRC encoding (encode_mrc_raw, write_mrc_raw; mc_mrc_encode, csrc/mrc_encode.hip over csrc/mrc_encode.h) without a
GPU: the names, the build list and the C ABI, the numpy restatement (tests/mrc_encode_reference.py) as the inverse of
tests/mrc_reference.py's decoder, the argument rules before any device is touched, the entry point's host checks with
fake pointers, the header's arithmetic, and the per-thread bodies of csrc/mrc_encode.h run on the CPU under the address
and undefined-behaviour sanitizers (tests/host_mrc_encode.cpp, a stand-alone program started as a child process)."""

import ctypes
import inspect
import os
import struct

import numpy as np
import pytest
import torch

import mrc_encode_reference as er
import mrc_reference as mr
from kernel_harness import assert_entry_point, run_host_program


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


# ------------------------------------------------------------------ names, the build list, the C ABI


def test_names_parameters_and_defaults(mc):
    from torch_motion_correction_amd import mrc

    for name in ("encode_mrc_raw", "write_mrc_raw"):
        assert name in mc.__all__ and getattr(mc, name) is getattr(mrc, name)

    def params(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    none = inspect.Parameter.empty
    assert params(mc.encode_mrc_raw) == [("movie", none), ("mode", None), ("flip_rows", False),
                                         ("return_statistics", False), ("device", None)]
    assert params(mc.write_mrc_raw) == [("path", none), ("movie", none), ("pixel_spacing", none), ("mode", None),
                                        ("flip_rows", False), ("device", None)]
    # what exists keeps its parameters
    assert params(mc.write_mrc) == [("path", none), ("image", none), ("pixel_spacing", none), ("dtype", torch.float32)]
    assert [f for f in mc.MrcMovie.__dataclass_fields__] == ["data", "offset", "shape", "mode", "swap",
                                                             "unsigned_bytes", "pixel_spacing"]


def test_sources_signatures_and_header_agree():
    from torch_motion_correction_amd import _build, _lib

    assert ("mrc_encode.hip", "mrc_encode", []) in _build.SOURCES
    assert _build.SOURCES[-1] == ("tiff_decode.hip", "tiff_decode", [])
    stems = [s[1] for s in _build.SOURCES]
    assert stems.index("mrc_encode") < stems.index("tiff_decode")
    for name in ("mrc_encode.hip", "mrc_encode.h"):
        assert os.path.exists(os.path.join(_build.CSRC, name))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert_entry_point("mc_mrc_encode", [vp, i32, i32, i32, i32, i32, i32, vp, i64, vp, vp, i64, vp])
    assert _lib.load().mc_abi_version() == 1
    rule = open(os.path.join(_build.CSRC, "mrc_encode.h")).read()
    assert "NOT been confirmed" in rule  # the 4-bit layout rests on the format descriptions; the header says so
    assert "hip/hip_runtime" not in rule and "THE SCRATCH RULE" in rule


# ------------------------------------------------------------------ the restatement is the decoder's inverse


@pytest.mark.parametrize("dtype,mode", er.KINDS)
@pytest.mark.parametrize("flip", [False, True])
def test_restatement_inverts_the_reference_decoder(dtype, mode, flip):
    for w in (1, 2, 31, 32, 33, 129):
        shape = (2, 3, w)
        px = er.pixels(dtype, mode, shape, seed=w)
        payload = er.encode(px, mode, flip_rows=flip)
        assert len(payload) == 2 * 3 * er.row_bytes(mode, w) == 2 * 3 * mr.row_bytes(mode, w)
        back = mr.decode(payload, shape, mode, unsigned_bytes=dtype == "u1", flip_rows=flip)
        assert back.dtype == (np.uint8 if mode == 101 or dtype == "u1" else np.int16)
        assert np.array_equal(back.astype(np.int64), px.astype(np.int64)), (w, flip)
        if not flip and mode != 101:  # and of the reference writer's rows
            file_px = px.astype(np.int8) if (dtype, mode) == ("i2", 0) else px.astype(np.uint16) if mode == 6 else px
            assert payload == mr.pack_rows(file_px, mode)
        if not flip and mode == 101:
            assert payload == mr.pack_rows(px.astype(np.uint8), 101, pad_nibble=0)
        table = er.statistics(px, mode)
        assert table.shape == (2, 5) and table.dtype == np.int64 and not table[:, 4].any()
        assert table[:, 0].min() == px.min() and table[:, 1].max() == px.max()
        assert int(table[:, 2].sum()) == int(px.astype(np.int64).sum())
        assert int(table[:, 3].sum()) == int((px.astype(np.int64) ** 2).sum())


@pytest.mark.parametrize("dtype", ["u1", "i2"])
def test_mode_101_padding_nibbles_are_zero(dtype):
    for w in (1, 31, 33, 129):
        px = np.full((2, 3, w), 15, dtype=dtype)
        rows = np.frombuffer(er.encode(px, 101), dtype=np.uint8).reshape(2, 3, (w + 1) // 2)
        assert (rows[:, :, -1] == 0x0F).all() and (rows[:, :, :-1] == 0xFF).all()


def test_out_of_range_samples_are_masked_and_counted():
    px = np.array([[[16, 3, 255]]], dtype=np.uint8)
    assert er.encode(px, 101) == bytes([0x30, 0x0F]) and er.statistics(px, 101)[0].tolist() == [3, 255, 274, 65290, 2]
    px = np.array([[[-1, 128, -129, 127]]], dtype=np.int16)
    assert er.encode(px, 0) == bytes([0xFF, 0x80, 0x7F, 0x7F]) and er.statistics(px, 0)[0, 4] == 2
    assert er.statistics(px, 6)[0, 4] == 2 and er.statistics(px, 1)[0, 4] == 0
    assert er.encode(px, 101) == bytes([0x0F, 0xFF]) and er.statistics(px, 101)[0, 4] == 4


# ------------------------------------------------------------------ argument rules, devices refused


def test_argument_rules_hold_before_any_device_is_touched(mc, monkeypatch, tmp_path):
    from torch_motion_correction_amd import mrc

    def touched(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    monkeypatch.setattr(mrc, "require_gpu", touched)
    monkeypatch.setattr(mrc, "device_scope", touched)
    u8, i16 = torch.zeros(2, 3, 4, dtype=torch.uint8), torch.zeros(2, 3, 4, dtype=torch.int16)
    path = tmp_path / "no.mrc"

    def refuse(match, movie=u8, spacing=1.0, **kw):
        with pytest.raises(ValueError, match=match):
            mc.encode_mrc_raw(movie, **kw)
        kw.pop("return_statistics", None)
        with pytest.raises(ValueError, match=match):
            mc.write_mrc_raw(path, movie, spacing, **kw)

    for bad in (np.zeros((2, 3, 4), np.uint8), torch.zeros(5, dtype=torch.uint8), torch.zeros(1, 2, 3, 4, dtype=torch.uint8),
                torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.float16),
                torch.zeros(3, 4, dtype=torch.int8), torch.zeros(3, 4, dtype=torch.bool), b"abc"):
        refuse(r"\(t, h, w\) or \(h, w\) tensor of dtype uint8 or int16", movie=bad)
    for bad in (torch.zeros(0, 3, 4, dtype=torch.uint8), torch.zeros(3, 0, dtype=torch.int16)):
        refuse("must not be empty", movie=bad)
    for bad in (1, 6, 2, 12, 3, -1, 100, "0", 0.0, True, [0]):
        refuse("mode must be None or one of 0, 101 for a movie of torch.uint8", mode=bad)
    for bad in (2, 12, 3, 7, -1, 102, "1", 1.0, False, (1,)):
        refuse("mode must be None or one of 1, 6, 0, 101 for a movie of torch.int16", movie=i16, mode=bad)
    for bad in (0, 1, None, "yes"):
        refuse("flip_rows must be a bool", flip_rows=bad)
        with pytest.raises(ValueError, match="return_statistics must be a bool"):
            mc.encode_mrc_raw(u8, return_statistics=bad)
    # a frame of 2^31 samples: a view without memory behind it
    refuse("2\\^31 samples", movie=torch.zeros(1, dtype=torch.uint8).expand(1, 1 << 16, 1 << 15))
    for bad in (0, -1.0, float("nan"), float("inf"), None, "1", True):
        with pytest.raises(ValueError, match="pixel_spacing must be"):
            mc.write_mrc_raw(path, u8, bad)
    # valid arguments get as far as the device, and no further here
    for movie, mode in ((u8, None), (u8, 0), (u8, 101), (u8[0], 101), (i16, None), (i16, 1), (i16, 6), (i16, 0), (i16, 101)):
        with pytest.raises(AssertionError, match="a device was touched"):
            mc.encode_mrc_raw(movie, mode=mode, flip_rows=True, return_statistics=True)
        with pytest.raises(AssertionError, match="a device was touched"):
            mc.write_mrc_raw(path, movie, 0.83, mode=mode)
    assert not path.exists()
    assert mrc._check_encode_args(u8, None, False) == (2, 3, 4, 0) and mrc._check_encode_args(i16[0], None, False) == (1, 3, 4, 1)


def test_entry_point_validates_on_the_host():
    """Fake device pointers and a null stream: every call below must answer before it touches or launches anything."""
    from torch_motion_correction_amd import _lib, mrc

    lib = _lib.load()
    p = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(4)]
    ARG, UNSUPPORTED = -1, -2

    def enc(movie=p[0], elem=1, t=2, h=3, w=5, mode=101, flip=0, payload=p[1], payload_bytes=18, stats=p[2],
            scratch=p[3], scratch_bytes=80):
        return lib.mc_mrc_encode(movie, elem, t, h, w, mode, flip, payload, payload_bytes, stats, scratch, scratch_bytes,
                                 None)

    assert mrc._scratch_bytes(1, 2, 3, 5) == 80  # 6 row-threads a frame: one workgroup
    assert enc(movie=None) == ARG and enc(payload=None) == ARG and enc(stats=None) == ARG and enc(scratch=None) == ARG
    assert enc(payload=p[0]) == ARG
    assert enc(t=0) == ARG and enc(h=0) == ARG and enc(w=-1) == ARG and enc(flip=2) == ARG and enc(flip=-1) == ARG
    assert enc(payload_bytes=-1) == ARG and enc(scratch_bytes=-1) == ARG
    assert enc(payload_bytes=17) == ARG  # 6 rows of 3 bytes
    assert enc(mode=0, payload_bytes=29) == ARG and enc(elem=2, mode=1, payload_bytes=59) == ARG
    assert enc(elem=2, mode=0, payload_bytes=29) == ARG and enc(elem=2, mode=101, payload_bytes=17) == ARG
    assert enc(scratch_bytes=79) == ARG
    assert enc(t=1 << 30, h=1 << 15, w=1 << 15, payload_bytes=1 << 62, scratch_bytes=1 << 40) == ARG  # no overflow
    assert enc(h=1 << 16, w=1 << 15, payload_bytes=1 << 40, scratch_bytes=1 << 40) == ARG  # 2^31 samples a frame
    # (1 << 16) - 1 rows of 1 << 15: below 2^31 samples, 1024 workgroups a frame: only the scratch is refused
    assert mrc._scratch_bytes(1, 2, (1 << 16) - 1, 1 << 15) == 2 * 1024 * 40
    assert enc(h=(1 << 16) - 1, w=1 << 15, payload_bytes=1 << 40, scratch_bytes=2 * 1024 * 40 - 1) == ARG
    assert enc(elem=2, mode=1, payload_bytes=60, movie=ctypes.c_void_p(0x100001)) == ARG
    assert enc(stats=ctypes.c_void_p(0x300004)) == ARG and enc(scratch=ctypes.c_void_p(0x400004)) == ARG
    for elem, mode in ((1, 1), (1, 6), (1, 2), (1, 12), (2, 2), (2, 12), (2, 3), (1, -1), (2, 100), (4, 2), (4, 0), (0, 0),
                       (3, 101), (-1, 1)):
        assert enc(elem=elem, mode=mode, payload_bytes=1000) == UNSUPPORTED, (elem, mode)
    assert enc(elem=4, mode=2, t=0) == ARG  # the sizes come before the pair


# ------------------------------------------------------------------ the header's arithmetic


@pytest.mark.parametrize("dtype,mode", er.KINDS)
def test_header_statistics_equal_float64_numpy(mc, dtype, mode):
    from torch_motion_correction_amd import mrc

    px = er.pixels(dtype, mode, (5, 37, 129), seed=3)
    got = mrc._header_statistics(torch.from_numpy(er.statistics(px, mode)), 37 * 129)
    want = er.header_statistics(px)
    assert got[:2] == want[:2] and all(isinstance(v, float) for v in got)
    # exact rationals rounded once against float64 sums of 23865 terms: far inside 1e-12
    assert got[2] == pytest.approx(want[2], rel=1e-12, abs=1e-12) and got[3] == pytest.approx(want[3], rel=1e-12)
    # the header is write_mrc's (the reference writer's) but for the mode, the statistics and IMOD's stamp
    header = mrc._header((5, 37, 129), mode, 0.83, got, unsigned_bytes=(dtype, mode) == ("u1", 0))
    assert bytes(header) == mr.header((5, 37, 129), mode, pixel_spacing=0.83, stats=got, label=mr.LABEL,
                                      imod=0 if (dtype, mode) == ("u1", 0) else None)
    assert struct.unpack_from("<3f", header, 76) + struct.unpack_from("<f", header, 216) == pytest.approx(want, rel=1e-6)
    assert struct.unpack_from("<4i", header, 0) == (129, 37, 5, mode)
    assert struct.unpack_from("<2i", header, 152) == ((mr.IMOD_STAMP, 0) if (dtype, mode) == ("u1", 0) else (0, 0))


def test_header_statistics_of_extreme_movies(mc):
    from torch_motion_correction_amd import mrc

    for dtype, mode, value in (("u1", 0, 255), ("u1", 101, 15), ("i2", 1, -32768), ("i2", 6, 32767), ("i2", 0, -128),
                               ("i2", 1, 0)):
        px = np.full((3, 64, 64), value, dtype=dtype)
        assert mrc._header_statistics(torch.from_numpy(er.statistics(px, mode)), 64 * 64) == \
            (float(value), float(value), float(value), 0.0)
    # a sum of squares beyond 2^53: 40 frames of 4096^2 samples of -32768, from the table alone
    n = 4096 * 4096
    table = torch.tensor([[-32768, -32768, -32768 * n, 32768 * 32768 * n, 0]] * 39
                         + [[-32768, -32767, -32768 * n + 1, 32768 * 32768 * n - 65535, 0]], dtype=torch.int64)
    dmin, dmax, dmean, rms = mrc._header_statistics(table, n)
    total = 40 * n
    assert (dmin, dmax) == (-32768.0, -32767.0) and -32768 < dmean < -32768 + 2 / total  # float64 resolves 1 / total here
    assert rms == pytest.approx(np.sqrt((1 - 1 / total) / total), rel=1e-12)  # one sample off by 1


# ------------------------------------------------------------------ the per-thread bodies on the CPU, sanitized


def _record(elem, mode, flip, shape, lead_in, lead_out, movie, want, table):
    t, h, w = shape
    return struct.pack("<10I", elem, mode, flip, t, h, w, lead_in, lead_out, len(movie), len(want)) + movie + want \
        + table.astype("<i8").tobytes()


def test_bodies_on_the_host_under_sanitizers(tmp_path):
    """csrc/mrc_encode.h -- the bodies mrc_encode.hip compiles for the device -- built for the host with
    -fsanitize=address,undefined into a program of its own and run as a child process: every kind, widths 1 .. 70, the
    movie and the payload starting at every offset 0 .. 15 of a 16-byte unit (an int16 movie at the even ones: the
    entry point refuses another), with and without flip_rows, with samples outside the mode's range.  The movie's and
    the payload's allocations are exact and their leads poisoned: a stray byte is a sanitizer report.  Payload and
    statistics are compared with the restatement's.  Nothing sanitized is loaded into this process."""
    records, seen = [], set()
    for dtype, mode in er.KINDS:
        elem = int(dtype[1])
        for w in range(1, 71):
            for a in range(16):
                lead_in, lead_out, flip = a - a % elem, (5 * a + w) % 16, (a // 2 + w) % 2
                shape = (2, 3, w)
                px = er.pixels(dtype, mode, shape, seed=a, spoil=(a + w) % 3)
                records.append(_record(elem, mode, flip, shape, lead_in, lead_out, px.tobytes(),
                                       er.encode(px, mode, bool(flip)), er.statistics(px, mode)))
                seen.add((dtype, mode, lead_in, flip))
                seen.add((dtype, mode, "out", lead_out))
    for dtype, mode in er.KINDS:
        for flip in (0, 1):
            assert all((dtype, mode, a - a % int(dtype[1]), flip) in seen for a in range(16))
        assert all((dtype, mode, "out", a) in seen for a in range(16))
    cases = tmp_path / "cases.bin"
    cases.write_bytes(b"".join(records))
    res = run_host_program("host_mrc_encode.cpp", tmp_path, cases)
    assert f"{len(records)} cases, 0 failures" in res.stdout
