"""MRC reading, decoding, orienting and writing (read_mrc, decode_mrc_raw, MrcMovie, orient_raw, write_mrc), without a
GPU: the names, the build list and the C ABI, read_mrc on files of tests/mrc_reference.py's writer, every refusal,
the argument rules before any device is touched, the entry points' host checks with fake pointers, write_mrc's bytes
and its round trip, and the per-thread bodies of csrc/mrc.h run on the CPU under the address and undefined-behaviour
sanitizers (tests/host_mrc.cpp, a stand-alone program started as a child process)."""

import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import mrc_reference as mr
from kernel_harness import assert_entry_point, run_host_program

MODES = (0, 1, 2, 6, 12, 101)


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def pixels_for(mode, shape, seed=0, signed_bytes=False):
    rng = np.random.default_rng([seed, mode, *shape])
    if mode == 101:
        return rng.integers(0, 16, shape, dtype=np.uint8)
    if mode == 0:
        return rng.integers(-128, 128, shape).astype(np.int8) if signed_bytes else \
            rng.integers(0, 256, shape, dtype=np.uint8)
    if mode == 1:
        return rng.integers(-32768, 32768, shape).astype(np.int16)
    if mode == 6:
        return rng.integers(0, 32768, shape).astype(np.uint16)
    if mode == 2:
        return rng.standard_normal(shape).astype(np.float32)
    return rng.standard_normal(shape).astype(np.float16)


# ------------------------------------------------------------------ names, the build list, the C ABI


def test_names_are_exported(mc):
    from torch_motion_correction_amd import mrc

    for name in ("read_mrc", "MrcMovie", "decode_mrc_raw", "orient_raw", "write_mrc"):
        assert name in mc.__all__ and getattr(mc, name) is getattr(mrc, name)
    assert [f for f in mc.MrcMovie.__dataclass_fields__] == ["data", "offset", "shape", "mode", "swap",
                                                             "unsigned_bytes", "pixel_spacing"]


def test_sources_signatures_and_header_agree():
    from torch_motion_correction_amd import _build

    assert ("mrc_decode.hip", "mrc_decode", []) in _build.SOURCES
    assert ("raw_orient.hip", "raw_orient", []) in _build.SOURCES
    assert _build.SOURCES[-1] == ("tiff_decode.hip", "tiff_decode", [])
    stems = [s[1] for s in _build.SOURCES]
    assert stems.index("mrc_decode") < stems.index("eer_render") and stems.index("raw_orient") < stems.index("eer_render")
    for name in ("mrc_decode.hip", "raw_orient.hip", "mrc.h"):
        assert os.path.exists(os.path.join(_build.CSRC, name))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert_entry_point("mc_mrc_decode", [vp, i64, i64, i32, i32, i32, i32, i32, i32, i32, vp, vp])
    assert_entry_point("mc_raw_orient", [vp, i32, i32, i32, i32, i32, i32, vp, vp])
    rule = open(os.path.join(_build.CSRC, "mrc.h")).read()
    assert "NOT been confirmed" in rule  # the 4-bit layout rests on the format descriptions; mrc.h says so


# ------------------------------------------------------------------ read_mrc


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("byte_order", ["<", ">"])
@pytest.mark.parametrize("stamp", [True, False])
def test_read_mrc(mc, tmp_path, mode, byte_order, stamp):
    shape = (3, 5, 7)
    px = pixels_for(mode, shape)
    path = tmp_path / "m.mrc"
    for nsymbt in (0, 7, 1024):
        raw = mr.write_mrc(path, px, mode, byte_order=byte_order, stamp=stamp, nsymbt=nsymbt, pixel_spacing=1.25,
                           trailing=b"xyz")
        got = mc.read_mrc(path)
        assert isinstance(got, mc.MrcMovie) and got.shape == shape and got.mode == mode
        assert got.offset == 1024 + nsymbt and got.swap is (byte_order == ">") and got.unsigned_bytes is False
        assert got.pixel_spacing == pytest.approx(1.25, rel=1e-6)
        assert got.data.dtype == torch.uint8 and got.data.dim() == 1 and bytes(got.data.numpy()) == raw
        payload = raw[got.offset:]
        want = mr.decode(payload, shape, mode, swap=got.swap)
        if mode == 6:
            assert np.array_equal(want.view(np.uint16), px)
        elif mode == 0:
            assert np.array_equal(want, px.view(np.int8).astype(np.int16))
        else:
            assert np.array_equal(want, px)


def test_read_mrc_mode_0_signedness_and_pixel_spacing(mc, tmp_path):
    px = pixels_for(0, (2, 3, 4))
    path = tmp_path / "m.mrc"
    for imod, unsigned in ((None, False), (0, True), (1, False), (2, True), (3, False)):
        mr.write_mrc(path, px, 0, imod=imod)
        got = mc.read_mrc(str(path))
        assert got.unsigned_bytes is unsigned, imod
        assert got.pixel_spacing is None
    # another stamp with the flag clear: not IMOD's, so signed
    mr.write_mrc(path, px, 0, overrides={"imodStamp": 12345, "imodFlags": 0})
    assert mc.read_mrc(path).unsigned_bytes is False
    # unsigned_bytes is a statement about mode 0 only
    mr.write_mrc(path, pixels_for(1, (2, 3, 4)), 1, imod=0)
    assert mc.read_mrc(path).unsigned_bytes is False
    mr.write_mrc(path, px, 0, pixel_spacing=0.83, overrides={"mx": 0})
    assert mc.read_mrc(path).pixel_spacing is None
    mr.write_mrc(path, px, 0, pixel_spacing=0.5, overrides={"mx": 8})  # cella.x = 4 * 0.5 over mx = 8
    assert mc.read_mrc(path).pixel_spacing == pytest.approx(0.25)


def test_read_mrc_refusals_name_the_field(mc, tmp_path):
    path = tmp_path / "bad.mrc"
    px = pixels_for(1, (2, 3, 4))

    def refuse(match, pixels=px, mode=1, **kw):
        mr.write_mrc(path, pixels, mode, **kw)
        with pytest.raises(ValueError, match=match):
            mc.read_mrc(path)

    for mode in (3, 4, 7, 5, 102, -1):
        refuse(f"mode {mode}\\b", mode=mode, payload=bytes(200))
    for bo in "<>":
        refuse("nx 0 ", overrides={"nx": 0}, byte_order=bo)
        refuse("ny -3 ", overrides={"ny": -3}, byte_order=bo)
        refuse("nz 0 ", overrides={"nz": 0}, byte_order=bo)
        refuse(r"mapc, mapr, maps = \(2, 1, 3\)", overrides={"mapc": 2, "mapr": 1}, byte_order=bo)
        refuse(r"mapc, mapr, maps = \(1, 2, 4\)", overrides={"maps": 4}, byte_order=bo)
        refuse("nsymbt -8 ", overrides={"nsymbt": -8}, byte_order=bo)
    refuse("imodFlags 16", pixels=pixels_for(0, (2, 3, 4)), mode=0, imod=16)
    refuse("imodFlags 17", pixels=pixels_for(0, (2, 3, 4)), mode=0, imod=17)
    refuse(r"mapc, mapr, maps = \(2, 1, 3\)", stamp=False, overrides={"mapc": 2, "mapr": 1})
    refuse("machine stamp 0x00 .* neither byte order", stamp=False, overrides={"maps": 7})
    # shorter than the header says: one byte short, and an extended header that is not there
    raw = mr.write_mrc(None, px, 1)
    path.write_bytes(raw[:-1])
    with pytest.raises(ValueError, match=f"{len(raw) - 1} bytes is shorter than the {len(raw)}"):
        mc.read_mrc(path)
    refuse("shorter than", overrides={"nsymbt": 16})
    refuse("shorter than", pixels=pixels_for(101, (2, 3, 5)), mode=101, overrides={"nx": 7})  # rows of 4 bytes, not 3
    path.write_bytes(raw[:1023])
    with pytest.raises(ValueError, match="1023 bytes is shorter than the 1024-byte MRC header"):
        mc.read_mrc(path)
    path.write_bytes(b"")
    with pytest.raises(ValueError, match="1024-byte"):
        mc.read_mrc(path)
    path.write_bytes(b"BZh91AY&SY" + bytes(2000))
    with pytest.raises(ValueError, match="bzip2-compressed MRC is not decoded"):
        mc.read_mrc(path)
    # trailing bytes are ignored, and the file is one
    path.write_bytes(raw + bytes(5))
    assert mc.read_mrc(path).shape == (2, 3, 4)


# ------------------------------------------------------------------ argument rules, devices refused


def test_argument_rules_hold_before_any_device_is_touched(mc, monkeypatch):
    from torch_motion_correction_amd import mrc

    def touched(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    monkeypatch.setattr(mrc, "require_gpu", touched)
    monkeypatch.setattr(mrc, "device_scope", touched)
    data = torch.zeros(1024 + 2 * 3 * 8, dtype=torch.uint8)
    ok = dict(data=data, offset=1024, shape=(2, 3, 4), mode=1)

    def refuse(match, **kw):
        with pytest.raises(ValueError, match=match):
            mc.decode_mrc_raw(**{**ok, **kw})

    for bad in (np.zeros(2000, np.uint8), torch.zeros(2000, dtype=torch.int16),
                torch.zeros(20, 100, dtype=torch.uint8), b"abc"):
        refuse("1-D uint8 tensor", data=bad)
    for bad in (-1, 1.0, None, True, "0"):
        refuse("offset must be an int >= 0", offset=bad)
    for bad in ((3, 4), (2, 3, 4, 5), (0, 3, 4), (2, -3, 4), (2, 3, 0), 24, (2.0, 3, 4), (True, 3, 4)):
        refuse(r"\(t, h, w\)", shape=bad)
    for bad in (3, 4, 7, 5, -1, 100, None, "1", 1.0, True, [1]):
        refuse("mode must be one of 0, 1, 2, 6, 12, 101", mode=bad)
    for name in ("swap", "unsigned_bytes", "flip_rows"):
        for bad in (0, 1, None, "yes"):
            refuse(f"{name} must be a bool", **{name: bad})
    refuse("offset 1025 .* = 1073 leaves the 1072 bytes", offset=1025)
    refuse("leaves the 1072 bytes", shape=(2, 3, 5))
    refuse("leaves the 1072 bytes", mode=2)
    refuse("leaves the 1072 bytes", shape=(4, 3, 9), mode=101)  # 4 x 3 rows of 5 bytes
    mc.mrc._check_decode_args(data, 1024, (4, 3, 8), 101, False, False, False)  # rows of 4 bytes: fits
    refuse("2\\^31 samples", shape=(1, 1 << 16, 1 << 15))
    # MrcMovie.decode goes through the same rules
    with pytest.raises(ValueError, match="leaves the 1072 bytes"):
        mc.MrcMovie(data, 1024, (2, 3, 4), 2, False, False, None).decode()
    with pytest.raises(ValueError, match="flip_rows must be a bool"):
        mc.MrcMovie(data, 1024, (2, 3, 4), 1, False, False, None).decode(flip_rows=1)

    x = torch.zeros(3, 4, 5, dtype=torch.int16)

    def refuse_orient(match, x=x, **kw):
        with pytest.raises(ValueError, match=match):
            mc.orient_raw(x, **kw)

    for bad in (np.zeros((4, 5), np.uint8), torch.zeros(5), torch.zeros(2, 3, 4, 5), torch.zeros(4, 5, dtype=torch.int32),
                torch.zeros(4, 5, dtype=torch.float64), torch.zeros(4, 5, dtype=torch.bool)):
        refuse_orient(r"\(h, w\) or \(n, h, w\)", x=bad)
    refuse_orient("must not be empty", x=torch.zeros(0, 4, dtype=torch.uint8))
    for bad in (1.0, None, "1", True):
        refuse_orient("rot90 must be an int", rot90=bad)
    for bad in ("up", 1, True, "UD", b"ud"):
        refuse_orient("flip must be None, 'ud' or 'lr'", flip=bad)
    # valid arguments get as far as the device, and no further here
    for kw in (dict(), dict(rot90=-7, flip="lr"), dict(rot90=10**12, flip="ud")):
        with pytest.raises(AssertionError, match="a device was touched"):
            mc.orient_raw(x, **kw)
    with pytest.raises(AssertionError, match="a device was touched"):
        mc.decode_mrc_raw(**ok)


def test_entry_points_validate_on_the_host():
    """Fake device pointers and a null stream: every call below must answer before it touches or launches anything."""
    from torch_motion_correction_amd import _lib

    lib = _lib.load()
    p = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(2)]
    ARG, UNSUPPORTED = -1, -2

    def dec(data=p[0], data_bytes=2000, offset=1024, t=2, h=3, w=4, mode=1, swap=0, ub=0, flip=0, out=p[1]):
        return lib.mc_mrc_decode(data, data_bytes, offset, t, h, w, mode, swap, ub, flip, out, None)

    assert dec(data=None) == ARG and dec(out=None) == ARG and dec(out=p[0]) == ARG
    assert dec(t=0) == ARG and dec(h=0) == ARG and dec(w=-1) == ARG and dec(offset=-1) == ARG and dec(data_bytes=-1) == ARG
    for mode in (3, 4, 7, 5, -1, 100, 102):
        assert dec(mode=mode) == ARG, mode
    assert dec(swap=2) == ARG and dec(ub=-1) == ARG and dec(flip=3) == ARG
    assert dec(data_bytes=1024 + 47) == ARG and dec(offset=1953) == ARG and dec(offset=3000) == ARG  # 48 bytes of rows
    assert dec(mode=2, data_bytes=1024 + 95) == ARG  # 96 bytes of rows
    assert dec(mode=101, w=5, data_bytes=1024 + 17) == ARG  # 6 rows of 3 bytes
    assert dec(t=1 << 30, h=1 << 15, w=1 << 15, data_bytes=1 << 60) == ARG  # 2^61 bytes of rows: no overflow
    for mode in (1, 6, 12, 0):  # int16 out
        assert dec(mode=mode, out=ctypes.c_void_p(0x200001)) == ARG, mode
    assert dec(mode=2, data_bytes=4000, out=ctypes.c_void_p(0x200002)) == ARG
    assert dec(h=1 << 16, w=1 << 15, data_bytes=1 << 40) == UNSUPPORTED
    assert dec(h=1 << 16, w=1 << 15, data_bytes=100) == UNSUPPORTED  # the size rule comes before the payload's
    assert dec(h=(1 << 16) - 1, w=1 << 15, data_bytes=100) == ARG  # one row below 2^31: only the payload is refused

    def ori(src=p[0], e=2, n=2, h=3, w=4, rot=1, flip=0, out=p[1]):
        return lib.mc_raw_orient(src, e, n, h, w, rot, flip, out, None)

    assert ori(src=None) == ARG and ori(out=None) == ARG and ori(out=p[0]) == ARG
    assert ori(n=0) == ARG and ori(h=0) == ARG and ori(w=-2) == ARG
    for e in (0, 3, 8, -1):
        assert ori(e=e) == ARG, e
    for rot in (-1, 4, 5):
        assert ori(rot=rot) == ARG, rot
    for flip in (-1, 3):
        assert ori(flip=flip) == ARG, flip
    assert ori(out=ctypes.c_void_p(0x200001)) == ARG and ori(src=ctypes.c_void_p(0x100001)) == ARG
    assert ori(e=4, out=ctypes.c_void_p(0x200002)) == ARG
    assert ori(h=1 << 16, w=1 << 15) == UNSUPPORTED and ori(e=1, rot=2, h=1 << 15, w=1 << 16) == UNSUPPORTED


# ------------------------------------------------------------------ write_mrc


@pytest.mark.parametrize("shape", [(6, 5), (3, 6, 5)])
@pytest.mark.parametrize("dtype,np_dtype,mode", [(torch.float32, "f4", 2), (torch.float16, "f2", 12)])
def test_write_mrc_bytes_and_round_trip(mc, tmp_path, shape, dtype, np_dtype, mode):
    # multiples of 1/8: sums are exact in float64 whatever their order
    image = np.random.default_rng(5).integers(-800, 800, shape).astype(np.float32) / 8
    path = tmp_path / "sum.mrc"
    assert mc.write_mrc(path, torch.from_numpy(image), 0.83, dtype=dtype) == path
    raw = path.read_bytes()
    want = mr.written_by_write_mrc(image, 0.83, np_dtype)
    assert raw[:1024] == want[:1024], [i for i in range(1024) if raw[i] != want[i]]
    assert raw == want
    nx, ny, nz, m = struct.unpack_from("<4i", raw, 0)
    assert (nz, ny, nx) == ((1,) + shape)[-3:] and m == mode
    assert struct.unpack_from("<3i", raw, 28) == (nx, ny, nz) and struct.unpack_from("<3i", raw, 64) == (1, 2, 3)
    assert struct.unpack_from("<3f", raw, 52) == (90.0, 90.0, 90.0)
    assert struct.unpack_from("<3f", raw, 40) == pytest.approx((nx * 0.83, ny * 0.83, nz * 0.83), rel=1e-6)
    assert struct.unpack_from("<2i", raw, 88) == (0, 0) and raw[104:108] == bytes(4)
    assert struct.unpack_from("<i", raw, 108)[0] == 20140 and raw[208:216] == b"MAP \x44\x44\x00\x00"
    assert struct.unpack_from("<i", raw, 220)[0] == 1 and b"torch_motion_correction_amd" in raw[224:304]
    written = image.astype(np_dtype).astype(np.float64)
    dmin, dmax, dmean = struct.unpack_from("<3f", raw, 76)
    assert (dmin, dmax) == (written.min(), written.max()) and dmean == pytest.approx(written.mean(), rel=1e-6)
    assert struct.unpack_from("<f", raw, 216)[0] == pytest.approx(written.std(), rel=1e-6)
    back = mc.read_mrc(mc.write_mrc(str(path), torch.from_numpy(image), 0.83, dtype=dtype))
    assert back.shape == ((1,) + shape)[-3:] and back.mode == mode and back.offset == 1024
    assert back.swap is False and back.unsigned_bytes is False and back.pixel_spacing == pytest.approx(0.83, rel=1e-6)
    got = mr.decode(bytes(back.data.numpy())[back.offset:], back.shape, back.mode)
    assert np.array_equal(got.reshape(shape), image.astype(np_dtype))


def test_write_mrc_argument_rules(mc, tmp_path):
    path = tmp_path / "x.mrc"
    img = torch.zeros(4, 5)
    for bad in (np.zeros((4, 5), np.float32), torch.zeros(4, 5, dtype=torch.int16), torch.zeros(5),
                torch.zeros(1, 2, 4, 5), torch.zeros(0, 5)):
        with pytest.raises(ValueError, match="image must be"):
            mc.write_mrc(path, bad, 1.0)
    for bad in (torch.float64, torch.int16, None):
        with pytest.raises(ValueError, match="dtype must be"):
            mc.write_mrc(path, img, 1.0, dtype=bad)
    for bad in (0, -1.0, float("nan"), float("inf"), None, "1", True):
        with pytest.raises(ValueError, match="pixel_spacing must be"):
            mc.write_mrc(path, img, bad)
    assert not path.exists()


# ------------------------------------------------------------------ the per-thread bodies on the CPU, sanitized


def _record(mode, swap, ub, flip, shape, lead_in, lead_out, payload, want):
    t, h, w = shape
    return struct.pack("<11I", mode, swap, ub, flip, t, h, w, lead_in, lead_out, len(payload), len(want)) \
        + payload + want


def test_bodies_on_the_host_under_sanitizers(tmp_path):
    """csrc/mrc.h -- the bodies mrc_decode.hip compiles for the device -- built for the host with
    -fsanitize=address,undefined into a program of its own and run as a child process: every mode and kind, rows whose
    first byte sits at every offset of a 16-byte unit (so head and tail are unaligned, and 2- and 4-byte samples are
    misaligned to themselves), widths around one and several units, odd widths in mode 101 with a padding nibble of
    15, with and without flip_rows.  Input and output allocations are exact and their leads poisoned: a stray byte
    is a sanitizer report.  Nothing sanitized is loaded into this process."""
    records = []
    kinds = [(0, 0, 1), (0, 0, 0), (1, 0, 0), (1, 1, 0), (6, 0, 0), (12, 1, 0), (2, 0, 0), (2, 1, 0), (101, 0, 0)]
    for mode, swap, ub in kinds:
        for w in (1, 2, 15, 16, 17, 31, 32, 33, 63, 65, 127, 200):
            for lead_in in range(17):
                shape = (2, 3, w)
                px = pixels_for(mode, shape, seed=lead_in, signed_bytes=not ub)
                payload = mr.pack_rows(px, mode, ">" if swap else "<", pad_nibble=15)
                flip = (lead_in + w) % 2
                want = mr.decode(payload, shape, mode, swap=bool(swap), unsigned_bytes=bool(ub), flip_rows=bool(flip))
                lead_out = (lead_in * want.dtype.itemsize) % 32
                records.append(_record(mode, swap, ub, flip, shape, lead_in, lead_out, payload, want.tobytes()))
    cases = tmp_path / "cases.bin"
    cases.write_bytes(b"".join(records))
    res = run_host_program("host_mrc.cpp", tmp_path, cases)
    assert f"{len(records)} cases, 0 failures" in res.stdout
