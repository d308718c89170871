"""TIFF LZW decode (decode_tiff_raw, read_tiff, TiffMovie), without a GPU: the names, parameter lists and defaults, the
header and the ctypes table on mc_tiff_decode, the codec rule's restatement (tests/tiff_reference.py) on the committed
libtiff-written files and on hand-made streams, read_tiff on TIFF and BigTIFF files written here and on the committed
files, every refusal before any device is touched, the entry point's host checks with fake pointers, and the
per-strip loop of csrc/tiff_lzw.h run on the CPU under the address and undefined-behaviour sanitizers
(tests/host_tiff_lzw.cpp, a stand-alone program started as a child process)."""

import ctypes
import inspect
import os
import re
import struct

import numpy as np
import pytest
import torch

import tiff_files
import tiff_reference as tr
from kernel_harness import assert_entry_point, run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff_lzw_libtiff.npz")
NAMES = ("u8_strips", "u8_long_strip", "u16", "f32", "u8_stored")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


def walk(raw):
    """The frames of a file libtiff wrote, by tiff_files.walk_ifds: independent of read_tiff -> [(strip offsets, strip
    byte counts, rows per strip, compression)] per frame."""
    frames = []
    for _, tags in tiff_files.walk_ifds(raw)[1]:
        value = {tag: values for tag, _, _, values in tags}
        frames.append((value[273], value[279], value[278][0], value[259][0]))
    return frames


def fixture_strips(golden, name):
    """-> (per frame the list of the strips' bytes, rows per strip, compression, pixels)"""
    raw = golden["file_" + name].tobytes()
    frames = walk(raw)
    strips = [[raw[o:o + n] for o, n in zip(fo, fn)] for fo, fn, _, _ in frames]
    h = golden["pixels_" + name].shape[1]
    return strips, min(frames[0][2], h), frames[0][3], golden["pixels_" + name]


# ------------------------------------------------------------------ the rule, pinned to libtiff (passes without the feature)


@pytest.mark.parametrize("name", NAMES[:4])
def test_restatement_decodes_the_libtiff_files(golden, name):
    strips, rps, compression, pixels = fixture_strips(golden, name)
    assert compression == 5 and len(strips) == pixels.shape[0]
    row_bytes = pixels.shape[2] * pixels.dtype.itemsize
    got, produced = tr.decode_movie(strips, pixels.shape[1:], rps, row_bytes)
    assert got == pixels.tobytes()
    assert np.array_equal(np.frombuffer(got, dtype=pixels.dtype).reshape(pixels.shape), pixels)


def test_the_fixtures_cover_what_they_are_for(golden):
    strips, rps, _, pixels = fixture_strips(golden, "u8_strips")
    assert pixels.shape[1] % rps != 0 and len(strips) == 3 and len(strips[0]) > 1 and pixels.shape[2] % 4 == 0
    strips, rps, _, pixels = fixture_strips(golden, "u8_long_strip")
    trace = []
    tr.decode_strip(strips[0][0], pixels[0].nbytes, trace)
    assert len(trace) > 4100 and {w for _, w, _ in trace} == {9, 10, 11, 12}
    assert sum(c == tr.CLEAR for c, _, _ in trace) >= 2  # the leading Clear and one inside the strip
    assert golden["pixels_u16"].dtype == np.uint16 and golden["pixels_f32"].dtype == np.float32
    assert fixture_strips(golden, "u8_stored")[2] == 1
    assert os.path.getsize(GOLDEN) < 200_000


# ------------------------------------------------------------------ names and the C ABI


def test_names_parameter_lists_and_defaults(mc):
    from torch_motion_correction_amd import tiff

    for name in ("decode_tiff_raw", "read_tiff", "TiffMovie"):
        assert name in mc.__all__ and getattr(mc, name) is getattr(tiff, name)
    sig = inspect.signature(mc.decode_tiff_raw)
    assert list(sig.parameters) == ["data", "offsets", "nbytes", "shape", "rows_per_strip", "compression", "dtype",
                                    "device"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(compression=5, dtype=torch.uint8, device=None)
    assert list(inspect.signature(mc.read_tiff).parameters) == ["path"]
    sig = inspect.signature(mc.TiffMovie.decode)
    assert list(sig.parameters) == ["self", "device"] and sig.parameters["device"].default is None
    assert [f for f in mc.TiffMovie.__dataclass_fields__] == ["data", "offsets", "nbytes", "shape", "rows_per_strip",
                                                              "compression", "dtype"]
    assert "Orientation" in mc.read_tiff.__doc__ and "stored order" in mc.read_tiff.__doc__


def test_header_signatures_and_build_agree(mc):
    from torch_motion_correction_amd import _build, _lib

    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    assert_entry_point("mc_tiff_decode", [vp, i64, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, i64, vp],
                       source=("tiff_decode.hip", "tiff_decode", []))
    assert _build.SOURCES[-1] == ("tiff_decode.hip", "tiff_decode", [])
    assert os.path.exists(os.path.join(_build.CSRC, "tiff_lzw.h"))
    assert _lib.load().mc_abi_version() == 1


# ------------------------------------------------------------------ the rule on hand-made streams


def pack(codes):
    """(code, width) pairs packed MSB-first"""
    bits = tr._Bits()
    for c, w in codes:
        bits.put(c, w)
    return bits.bytes()


def test_bit_order_and_the_first_codes():
    # Clear, 'A', 'B', EOI at 9 bits: 100000000 001000001 001000010 100000001
    s = pack([(256, 9), (65, 9), (66, 9), (257, 9)])
    assert s == bytes([0b10000000, 0b00010000, 0b01001000, 0b01010000, 0b00010000])
    assert tr.decode_strip(s, 10) == (b"AB", "eoi")
    # no leading Clear: the decoder starts cleared
    assert tr.decode_strip(pack([(65, 9), (66, 9), (258, 9), (257, 9)]), 10) == (b"ABAB", "eoi")
    # no EOI: the stream ends where fewer than `width` bits are left (here 5 bits of padding)
    assert tr.decode_strip(pack([(256, 9), (65, 9), (66, 9)]), 10) == (b"AB", "bits")
    # the expected size ends it, clipping a string; trailing bytes are ignored
    s = pack([(256, 9), (65, 9), (66, 9), (258, 9), (258, 9), (257, 9)]) + b"\xff" * 7
    assert tr.decode_strip(s, 5) == (b"ABABA", "full") and tr.decode_strip(s, 6) == (b"ABABAB", "full")
    assert tr.decode_strip(s, 2) == (b"AB", "full") and tr.decode_strip(s, 0) == (b"", "full")


def test_kwkwk():
    # 'A', then 258 while next == 258: AA; then 259 while next == 259: AAA
    assert tr.decode_strip(pack([(256, 9), (65, 9), (258, 9), (259, 9), (257, 9)]), 99) == (b"A" * 6, "eoi")
    # the encoder gets there by itself on a constant strip: every code after the first is KwKwK
    s = tr.encode_strip(bytes(300))
    trace = []
    assert tr.decode_strip(s, 300, trace) == (bytes(300), "full")
    data = [(c, n) for c, _, n in trace if c != tr.CLEAR]
    assert data[0][0] == 0 and all(c == n for c, n in data[1:-1]) and len(data) > 20


def test_malformed_codes_stop_where_the_rule_says():
    # a table code with no previous code: at the start, and after a Clear
    assert tr.decode_strip(pack([(300, 9), (65, 9)]), 10) == (b"", "malformed")
    assert tr.decode_strip(pack([(256, 9), (300, 9), (65, 9)]), 10) == (b"", "malformed")
    assert tr.decode_strip(pack([(256, 9), (258, 9)]), 10) == (b"", "malformed")  # KwKwK needs a previous code too
    assert tr.decode_strip(pack([(256, 9), (65, 9), (256, 9), (258, 9)]), 10) == (b"A", "malformed")
    # a code beyond next: what came before stays
    assert tr.decode_strip(pack([(256, 9), (65, 9), (66, 9), (260, 9), (67, 9)]), 10) == (b"AB", "malformed")
    assert tr.decode_strip(pack([(256, 9), (65, 9), (66, 9), (259, 9), (67, 9)]), 10)[1] != "malformed"  # 259 == next
    # old-style (LSB-first) streams are not recognised: the same codes packed LSB-first end within a few codes, far
    # short of the strip's size, which decode_tiff_raw reports as a malformed strip
    for seed in range(4):
        data = np.random.default_rng(seed).poisson(1.0, 600).astype(np.uint8).tobytes()
        trace = []
        tr.decode_strip(tr.encode_strip(data), 600, trace)
        value = n = 0
        for c, w, _ in trace + [(tr.EOI, trace[-1][1], 0)]:
            value |= c << n
            n += w
        got, why = tr.decode_strip(value.to_bytes((n + 7) // 8, "little"), 600)
        assert len(got) < 20 and why in ("malformed", "eoi") and got != data[:len(got)]
    # fewer than 9 bits
    assert tr.decode_strip(b"", 10) == (b"", "bits") and tr.decode_strip(b"\x80", 10) == (b"", "bits")


def test_the_width_changes_at_exactly_510_1022_and_2046():
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 6000, dtype=np.uint8).tobytes()  # noise: nearly every code adds an entry
    s = tr.encode_strip(data)
    trace = []
    assert tr.decode_strip(s, len(data), trace) == (data, "full")
    first = {}
    for c, w, n in trace:
        assert w == (9 if n <= 510 else 10 if n <= 1022 else 11 if n <= 2046 else 12), (c, w, n)
        first.setdefault(w, n)
    # a code read while next is 510 still has 9 bits; the one after it (next == 511) has 10 -- one entry EARLIER
    # than a decoder without the early change would switch
    assert {(w, n) for _, w, n in trace} >= {(9, 510), (10, 511), (10, 1022), (11, 1023), (11, 2046), (12, 2047)}
    assert first[10] == 511 and first[11] == 1023 and first[12] == 2047
    assert any(c == tr.CLEAR and n >= 4093 for c, _, n in trace)  # the libtiff-style Clear, before the table is full


def test_the_table_full_without_clear():
    rng = np.random.default_rng(6)
    data = rng.integers(0, 256, 9000, dtype=np.uint8).tobytes()
    s = tr.encode_strip(data, defer_clear=200)
    trace = []
    assert tr.decode_strip(s, len(data), trace) == (data, "full")
    full = [(c, w) for c, w, n in trace if n == tr.TABLE]
    assert len(full) >= 201 and all(w == 12 for _, w in full) and full[200][0] == tr.CLEAR
    assert max(n for _, _, n in trace) == tr.TABLE  # nothing is added beyond 4095
    # the encoder's other switches decode to the same bytes
    for kw in (dict(leading_clear=False), dict(eoi=False), dict(clear_at=100), dict(leading_clear=False, eoi=False)):
        assert tr.decode_strip(tr.encode_strip(data, **kw), len(data))[0] == data, kw
    trace = []
    tr.decode_strip(tr.encode_strip(data, clear_at=100), len(data), trace)
    assert sum(c == tr.CLEAR for c, _, _ in trace) == 1 + (len(trace) - 2) // 101
    assert tr.encode_strip(data, leading_clear=False)[0] == data[0] >> 1  # the first code is the first byte


# ------------------------------------------------------------------ containers


def movie_u8(seed, t, h, w):
    return np.random.default_rng(seed).poisson(1.0, (t, h, w)).astype(np.uint8)


@pytest.mark.parametrize("big,byte_order,array_type,rps", [(False, "<", 3, 5), (False, ">", 4, 37), (True, "<", 16, 5),
                                                           (True, ">", 3, 12), (False, "<", 4, 12), (True, ">", 16, 40)])
def test_read_tiff_on_both_containers(mc, tmp_path, big, byte_order, array_type, rps):
    """SHORT, LONG and LONG8 strip arrays, inline (one strip; two SHORTs; up to four SHORTs or two LONGs in BigTIFF)
    and out of line, in both byte orders."""
    movie = movie_u8(3, 3, 37, 20)
    strips = tr.encode_movie(movie, rps)
    path = tmp_path / "movie.tif"
    offsets, nbytes = tr.write_tiff(path, strips, (37, 20), rps, big=big, byte_order=byte_order,
                                    array_type=array_type)
    got = mc.read_tiff(path)
    assert isinstance(got, mc.TiffMovie) and got.shape == (37, 20) and got.rows_per_strip == min(rps, 37)
    assert got.compression == 5 and got.dtype == torch.uint8
    assert got.offsets == offsets and got.nbytes == nbytes and len(got.offsets[0]) == -(-37 // rps)
    assert got.data.dtype == torch.uint8 and got.data.dim() == 1 and got.data.numel() == os.path.getsize(path)
    raw = bytes(got.data.tolist())
    for fo, fn, fs in zip(got.offsets, got.nbytes, strips):
        assert [raw[o:o + n] for o, n in zip(fo, fn)] == fs
    # absent RowsPerStrip means one strip; absent SampleFormat means unsigned; Orientation is ignored
    one = tr.encode_movie(movie, 37)
    tr.write_tiff(path, one, (37, 20), 37, big=big, byte_order=byte_order, array_type=array_type,
                  overrides={i: {278: None, 339: None, 274: (3, 1, 4)} for i in range(3)})
    got = mc.read_tiff(str(path))
    assert got.rows_per_strip == 37 and got.dtype == torch.uint8 and [len(f) for f in got.offsets] == [1, 1, 1]
    # libtiff's "the whole frame": RowsPerStrip 2^32 - 1
    tr.write_tiff(path, one, (37, 20), 2**32 - 1, big=big, byte_order=byte_order, array_type=array_type)
    assert mc.read_tiff(path).rows_per_strip == 37


def test_read_tiff_sample_types(mc, tmp_path):
    path = tmp_path / "m.tif"
    for bits, fmt, dtype, np_dtype in ((16, 2, torch.int16, np.int16), (16, 1, torch.uint16, np.uint16),
                                       (32, 3, torch.float32, np.float32)):
        movie = np.arange(2 * 6 * 5).reshape(2, 6, 5).astype(np_dtype)
        tr.write_tiff(path, tr.encode_movie(movie, 4), (6, 5), 4, bits=bits, sample_format=fmt)
        got = mc.read_tiff(path)
        assert got.dtype == dtype and got.shape == (6, 5) and got.rows_per_strip == 4
    stored = [[bytes(s) for s in tr.strips_of(f.tobytes(), 5, 4)] for f in movie_u8(1, 2, 6, 5)]
    tr.write_tiff(path, stored, (6, 5), 4, compression=1)
    assert mc.read_tiff(path).compression == 1


@pytest.mark.parametrize("name", NAMES)
def test_read_tiff_on_the_committed_files(mc, golden, tmp_path, name):
    path = tmp_path / (name + ".tif")
    path.write_bytes(golden["file_" + name].tobytes())
    pixels = golden["pixels_" + name]
    got = mc.read_tiff(path)
    frames = walk(golden["file_" + name].tobytes())
    assert got.shape == pixels.shape[1:] and len(got.offsets) == pixels.shape[0]
    assert got.offsets == [f[0] for f in frames] and got.nbytes == [f[1] for f in frames]
    assert got.rows_per_strip == min(frames[0][2], pixels.shape[1]) and got.compression == frames[0][3]
    assert got.dtype == {"u8_strips": torch.uint8, "u8_long_strip": torch.uint8, "u16": torch.uint16,
                         "f32": torch.float32, "u8_stored": torch.uint8}[name]
    if name == "u8_stored":  # the strips are the rows
        raw = bytes(got.data.tolist())
        assert b"".join(raw[o:o + n] for fo, fn in zip(got.offsets, got.nbytes) for o, n in zip(fo, fn)) == \
            pixels.tobytes()


@pytest.mark.parametrize("big", [False, True])
def test_read_tiff_refusals_name_the_frame_and_the_tag(mc, tmp_path, big):
    movie = movie_u8(4, 3, 12, 10)
    strips = tr.encode_movie(movie, 5)
    path = tmp_path / "bad.tif"

    def refuse(match, strips=strips, shape=(12, 10), rps=5, **kw):
        tr.write_tiff(path, strips, shape, rps, big=big, **kw)
        with pytest.raises(ValueError, match=match):
            mc.read_tiff(path)

    for comp, word in ((8, "deflate"), (32946, "deflate"), (7, "JPEG"), (65001, "EER"), (2, "not supported")):
        refuse(f"frame 0: Compression {comp} .*{word}", compression=comp)
    refuse("frame 1: Compression 8 ", overrides={1: {259: (3, 1, 8)}})
    refuse("frame 0: Predictor 2", overrides={0: {317: (3, 1, 2)}})
    refuse("frame 2: Predictor 3", overrides={2: {317: (3, 1, 3)}})
    refuse("frame 0: FillOrder 2", overrides={0: {266: (3, 1, 2)}})
    refuse("frame 1: SamplesPerPixel 3", overrides={1: {277: (3, 1, 3)}})
    refuse("frame 0: BitsPerSample has 3 values; SamplesPerPixel", overrides={0: {258: (3, 3, [8, 8, 8]),
                                                                                  277: (3, 1, 3)}})
    for tag, name in ((322, "TileWidth"), (323, "TileLength"), (324, "TileOffsets"), (325, "TileByteCounts")):
        refuse(f"frame 1: {name} .*tiled", overrides={1: {tag: (4, 1, 16)}})
    for bits in (1, 4, 12, 32, 64):
        refuse(f"frame 0: BitsPerSample {bits} ", bits=bits)
    refuse("frame 0: BitsPerSample 1 ", overrides={i: {258: None} for i in range(3)})  # the default
    refuse("frame 0: BitsPerSample 8 with SampleFormat 2", sample_format=2)
    refuse("frame 0: BitsPerSample 16 with SampleFormat 3", bits=16, sample_format=3)
    refuse("frame 0: BitsPerSample 16 in a big-endian", bits=16, sample_format=2, byte_order=">")
    refuse("frame 0: BitsPerSample 32 in a big-endian", bits=32, sample_format=3, byte_order=">")
    refuse("frame 1: ImageWidth 11 differs", overrides={1: {256: (4, 1, 11)}})
    refuse("frame 2: ImageLength 13 differs", overrides={2: {257: (4, 1, 13)}})
    refuse("frame 1: Compression 1 differs", overrides={1: {259: (3, 1, 1)}})
    refuse("frame 1: BitsPerSample / SampleFormat .* differs", overrides={1: {258: (3, 1, 16)}})
    refuse("frame 2: RowsPerStrip 4 differs", overrides={2: {278: (4, 1, 4)}})
    refuse("frame 0: StripOffsets has 3 and StripByteCounts 3 values, but 12 rows in strips of 3 are 4 strips", rps=3)
    refuse("frame 1: StripOffsets has 2 and StripByteCounts 3", overrides={1: {273: (4, 2, [8, 9])}})
    for tag, name in ((256, "ImageWidth"), (257, "ImageLength"), (259, "Compression"), (273, "StripOffsets"),
                      (279, "StripByteCounts")):
        refuse(f"frame 1: {name} is missing", overrides={1: {tag: None}})
    refuse("frame 0: ImageWidth has TIFF type 5", overrides={0: {256: (5, 1, 64)}})
    refuse("frame 0: StripOffsets has TIFF type 1", overrides={0: {273: (1, 3, 64)}})
    refuse("frame 2, strip 1: StripOffsets \\+ StripByteCounts", overrides={2: {279: (4, 3, [5, 10**6, 5])}})
    refuse("frame 1: StripByteCounts: its 3 values at offset .* leave the file",
           overrides={1: {279: (16, 3, 10**7)}})
    refuse("frame 0: ImageLength x ImageWidth .* is empty", overrides={i: {256: (4, 1, 0)} for i in range(3)})
    refuse("frame 3: the IFD chain loops", loop=True)
    size = os.path.getsize(path)
    raw = bytearray(path.read_bytes())
    # the first IFD's offset past the end of the file
    struct.pack_into("<Q" if big else "<I", raw, 8 if big else 4, size + 10)
    path.write_bytes(raw)
    with pytest.raises(ValueError, match="frame 0: its IFD lies outside the file"):
        mc.read_tiff(path)
    path.write_bytes(b"")
    with pytest.raises(ValueError, match="empty"):
        mc.read_tiff(path)
    path.write_bytes(b"II" + (44).to_bytes(2, "little") + bytes(12))
    with pytest.raises(ValueError, match="magic 44"):
        mc.read_tiff(path)
    path.write_bytes(b"PK\x03\x04" + bytes(12))
    with pytest.raises(ValueError, match="not a TIFF"):
        mc.read_tiff(path)
    path.write_bytes((b"II+\x00\x08\x00\x00\x00" + bytes(8)) if big else (b"II*\x00" + bytes(4)))
    with pytest.raises(ValueError, match="no frame"):
        mc.read_tiff(path)


# ------------------------------------------------------------------ argument rules, devices refused


def test_argument_rules_hold_before_any_device_is_touched(mc, monkeypatch):
    from torch_motion_correction_amd import tiff

    def touched(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    monkeypatch.setattr(tiff, "require_gpu", touched)
    monkeypatch.setattr(tiff, "device_scope", touched)
    data = torch.zeros(100, dtype=torch.uint8)
    ok = dict(data=data, offsets=[[0, 10], [20, 30]], nbytes=[[10, 10], [10, 10]], shape=(8, 8), rows_per_strip=5)

    def refuse(match, **kw):
        with pytest.raises(ValueError, match=match):
            mc.decode_tiff_raw(**{**ok, **kw})

    for bad in (np.zeros(100, np.uint8), torch.zeros(100, dtype=torch.int16), torch.zeros(10, 10, dtype=torch.uint8),
                b"abc"):
        refuse("1-D uint8 tensor", data=bad)
    for bad in ((8,), (8, 8, 8), (0, 8), (8, -1), 8, (8.0, 8)):
        refuse(r"\(h, w\)", shape=bad)
    for bad in (torch.int32, torch.float64, torch.float16, None, "uint8"):
        refuse("dtype must be", dtype=bad)
    for bad, word in ((8, "deflate"), (32946, "deflate"), (7, "JPEG"), (65001, "EER"), (0, "got 0"),
                      (True, "got True"), (None, "got None")):
        refuse(f"compression must be 5 .*{word}", compression=bad)
    for bad in (0, -1, 2.0, None, True, "3"):
        refuse("rows_per_strip must be an int >= 1", rows_per_strip=bad)
    refuse("2\\^31 bytes", shape=(1 << 16, 1 << 16), rows_per_strip=1 << 15)
    refuse("2\\^31 bytes", shape=(1 << 16, 1 << 15), rows_per_strip=1 << 14, dtype=torch.float32)
    refuse("same frames", offsets=[[0, 10]])
    refuse("same frames", offsets=[], nbytes=[])
    refuse("sequences", offsets=5)
    refuse("sequences", offsets=[0, 10], nbytes=[10, 10])  # one list per frame, not one int
    refuse("an offset must be an int >= 0", offsets=[[0, -1], [20, 30]])
    refuse("a byte count must be an int >= 0", nbytes=[[10, 1.5], [10, 10]])
    refuse("frame 1: 1 offsets and 2 byte counts, but 8 rows in strips of 5 are 2 strips", offsets=[[0, 10], [20]])
    refuse("frame 0: 2 offsets and 2 byte counts, but 8 rows in strips of 3 are 3 strips", rows_per_strip=3)
    refuse("frame 1, strip 1: offset 95, 10 bytes leaves the 100 bytes", offsets=[[0, 10], [20, 95]])
    refuse("frame 0, strip 1: offset 10, 91 bytes", nbytes=[[10, 91], [10, 10]])
    # TiffMovie.decode goes through the same rules
    movie = mc.TiffMovie(data=data, offsets=[[0]], nbytes=[[101]], shape=(8, 8), rows_per_strip=8, compression=5,
                         dtype=torch.uint8)
    with pytest.raises(ValueError, match="frame 0, strip 0"):
        movie.decode()
    with pytest.raises(ValueError, match="deflate"):
        mc.TiffMovie(data, [[0]], [[10]], (8, 8), 8, 8, torch.uint8).decode()


def test_entry_point_validates_on_the_host():
    """Fake device pointers and a null stream: every call below must answer before it touches or launches anything."""
    from torch_motion_correction_amd import _lib

    lib = _lib.load()
    p = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(4)]
    ARG, UNSUPPORTED = -1, -2
    i64x = lambda v: (ctypes.c_int64 * len(v))(*v)  # noqa: E731

    def call(data=p[0], data_bytes=1000, offsets=(0, 100, 200, 300), nbytes=(100, 100, 100, 100), n=2, spf=2, h=8,
             row_bytes=8, rps=5, comp=5, out=p[1], produced=p[2], scratch=p[3], scratch_bytes=1 << 20):
        off = None if offsets is None else i64x(offsets)
        nb = None if nbytes is None else i64x(nbytes)
        return lib.mc_tiff_decode(data, data_bytes, off, nb, n, spf, h, row_bytes, rps, comp, out, produced, scratch,
                                  scratch_bytes, None)

    for name in ("data", "offsets", "nbytes", "out", "produced", "scratch"):
        assert call(**{name: None}) == ARG, name
    assert call(n=0) == ARG and call(spf=0) == ARG and call(h=0) == ARG and call(row_bytes=0) == ARG
    assert call(rps=0) == ARG and call(rps=-2) == ARG and call(data_bytes=-1) == ARG and call(scratch_bytes=-1) == ARG
    for comp in (8, 32946, 7, 65001, 0, 2):
        assert call(comp=comp) == UNSUPPORTED, comp
    assert call(rps=9) == ARG  # more rows than the frame has
    assert call(spf=1) == ARG and call(spf=3) == ARG and call(rps=4, spf=3) == ARG  # ceil(8 / 5) = 2, ceil(8 / 4) = 2
    assert call(produced=ctypes.c_void_p(0x300002)) == ARG and call(scratch=ctypes.c_void_p(0x400004)) == ARG
    assert call(offsets=(0, -1, 200, 300)) == ARG and call(nbytes=(100, -5, 100, 100)) == ARG
    assert call(offsets=(0, 100, 200, 901)) == ARG and call(offsets=(0, 100, 2000, 300)) == ARG  # leaves the buffer
    assert call(h=1 << 20, rps=1 << 16, spf=16, row_bytes=1 << 15, offsets=(0,) * 32, nbytes=(1,) * 32) == UNSUPPORTED
    assert call(h=1 << 20, rps=(1 << 16) - 1, spf=17, row_bytes=1 << 15, offsets=(0,) * 34, nbytes=(1,) * 34,
                scratch_bytes=0) == ARG  # one byte below 2^31: only the scratch is refused
    assert call(scratch_bytes=16 * 4 - 1) == ARG  # 16 bytes per strip
    assert call(comp=1, scratch_bytes=16 * 4 - 1) == ARG


# ------------------------------------------------------------------ the per-strip loop on the CPU, sanitized


def _record(kind, stream, expected, want):
    return struct.pack("<4I", kind, len(stream), expected, len(want)) + stream + want


def test_strip_loop_on_the_host_under_sanitizers(golden, tmp_path):
    """csrc/tiff_lzw.h -- the loop tiff_decode.hip compiles for the device -- is built for the host with
    -fsanitize=address,undefined into a program of its own and run as a child process on exactly-sized buffers: every
    strip of the committed libtiff files, encoder-made strips of every option, the malformed strips of
    tests/test_tiff_decode.py, a short strip cut at every length, each strip also decoded into fewer bytes than it
    holds, garbage, the empty and every one-byte stream.  Nothing sanitized is loaded into this process."""
    records = []
    for name in NAMES[:4]:
        strips, rps, _, pixels = fixture_strips(golden, name)
        row_bytes = pixels.shape[2] * pixels.dtype.itemsize
        for frame, px in zip(strips, pixels):
            for s, want in zip(frame, tr.strips_of(px.tobytes(), row_bytes, rps)):
                records.append(_record(0, s, len(want), want))
    rng = np.random.default_rng(8)
    noise = rng.integers(0, 256, 9000, dtype=np.uint8).tobytes()
    periodic = bytes([3, 7] * 3000)
    for data in (noise, periodic, bytes(5000), rng.poisson(1.0, 7000).astype(np.uint8).tobytes()):
        for kw in (dict(), dict(leading_clear=False), dict(eoi=False), dict(defer_clear=300), dict(clear_at=50)):
            records.append(_record(0, tr.encode_strip(data, **kw), len(data), data))
    short = rng.poisson(1.0, 400).astype(np.uint8).tobytes()
    records.append(_record(1, tr.encode_strip(short), len(short), short))
    records.append(_record(1, tr.encode_strip(bytes(700), eoi=False), 700, bytes(700)))
    # malformed strips: the reference says how far they get
    for s in (tr.encode_strip(noise)[:4000], pack([(256, 9), (300, 9), (65, 9)]), pack([(65, 9), (66, 9), (260, 9)]),
              pack([(256, 9), (65, 9), (257, 9), (66, 9)])):
        want, why = tr.decode_strip(s, len(noise))
        assert why != "full"
        records.append(_record(0, s, len(noise), want))
    cases = tmp_path / "cases.bin"
    cases.write_bytes(b"".join(records))
    res = run_host_program("host_tiff_lzw.cpp", tmp_path, cases)
    n_cases = int(re.search(r"(\d+) cases, 0 failures", res.stdout).group(1))
    assert n_cases > 5 * len(records)
