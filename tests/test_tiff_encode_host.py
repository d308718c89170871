"""TIFF LZW encode and TIFF writing (encode_tiff_raw, write_tiff), without a GPU: the names and the C ABI, the size
bound slot_bytes against the reference encoder (tests/tiff_reference.py::encode_strip) and the closed form, the
per-strip loop of csrc/tiff_lzw_encode.h run on the CPU under the address and undefined-behaviour sanitizers
(tests/host_tiff_lzw_encode.cpp, a stand-alone program started as a child process) and compared byte for byte with the
reference encoder, the entry points' host checks with fake pointers, the argument rules before any device is touched,
and write_tiff's files of stored strips read back by a struct walk of their IFDs and by read_tiff."""

import ctypes
import inspect
import os
import re
import struct

import numpy as np
import pytest
import torch

import tiff_reference as tr
from kernel_harness import assert_entry_point, header_parameters, run_host_program
from tiff_files import walk_ifds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff_lzw_libtiff.npz")
NAMES = ("u8_strips", "u8_long_strip", "u16", "f32")


@pytest.fixture(scope="module")
def mc():
    import torch_motion_correction_amd as m

    return m


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


def closed_form(n):
    """at most n data codes, one leading Clear, one Clear per 3835 added entries, EOI; 12 bits each"""
    codes = n + n // 3835 + 2
    return (12 * codes + 7) // 8


def distinct_pairs(n):
    """n bytes in which no pair of neighbours repeats within 65536 bytes (a de Bruijn sequence of order 2 over the
    256 byte values, repeated): no table entry is ever used, every code is a single byte -- the worst case"""
    seq, a = [], [0, 0, 0]

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, 256):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    assert len(seq) == 65536
    return bytes((seq * (n // 65536 + 1))[:n])


def slot_bytes(n):
    from torch_motion_correction_amd import tiff

    return tiff._slot_bytes(n)


# ------------------------------------------------------------------ names and the C ABI


def test_names_parameter_lists_and_defaults(mc):
    from torch_motion_correction_amd import tiff

    for name in ("encode_tiff_raw", "write_tiff"):
        assert name in mc.__all__ and getattr(mc, name) is getattr(tiff, name)
    sig = inspect.signature(mc.encode_tiff_raw)
    assert list(sig.parameters) == ["movie", "rows_per_strip", "compression", "device"]
    assert [p.default for p in sig.parameters.values()][1:] == [None, 5, None]
    sig = inspect.signature(mc.write_tiff)
    assert list(sig.parameters) == ["path", "movie", "rows_per_strip", "compression", "bigtiff", "device"]
    assert [p.default for p in sig.parameters.values()][2:] == [None, 5, None, None]


def test_header_signatures_and_build_agree():
    from torch_motion_correction_amd import _build

    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    source = ("tiff_encode.hip", "tiff_encode", [])
    assert_entry_point("mc_tiff_encode", [vp, i32, i32, i32, i32, i32, vp, i64, i64, vp, vp], source)
    assert_entry_point("mc_tiff_pack", [vp, i64, vp, vp, i64, vp, i64, vp], source)
    assert_entry_point("mc_tiff_encode_slot_bytes", [i64, ctypes.POINTER(i64)], source)
    assert header_parameters("mc_tiff_encode_slot_bytes") == ["long long strip_bytes", "long long* slot_bytes"]
    assert os.path.exists(os.path.join(_build.CSRC, "tiff_lzw_encode.h"))


# ------------------------------------------------------------------ the size bound


def test_slot_bytes_bounds_the_reference_encoder():
    rng = np.random.default_rng(1)
    worst = distinct_pairs(70000)
    trace = []
    assert tr.decode_strip(tr.encode_strip(worst[:9000]), 9000, trace) == (worst[:9000], "full")
    assert all(c < 258 for c, _, _ in trace)  # nothing but single bytes and Clears: the worst case
    assert sum(c == tr.CLEAR for c, _, _ in trace) == 1 + 9000 // 3836
    cases = [bytes(n) for n in range(301)] + [worst[:n] for n in range(301)]
    for n in (301, 1000, 3835, 3836, 3837, 7672, 20000, 65536, 70000):
        cases += [bytes(n), worst[:n], rng.integers(0, 256, n, dtype=np.uint8).tobytes(),
                  rng.poisson(1.0, n).astype(np.uint8).tobytes()]
    for data in cases:
        n = len(data)
        got = slot_bytes(n)
        assert got >= closed_form(n) >= len(tr.encode_strip(data)), n
        assert got % 16 == 0 and got < closed_form(n) + 16
    assert slot_bytes(0) >= 3 == len(tr.encode_strip(b""))
    assert slot_bytes(2**31 - 1) >= closed_form(2**31 - 1)
    # the worst case comes close: the bound is not slack by more than the narrow codes at the start of each table
    assert len(tr.encode_strip(worst)) > 0.93 * closed_form(70000)


def test_slot_bytes_entry_point():
    from torch_motion_correction_amd import _lib

    lib, out = _lib.load(), ctypes.c_int64(-7)
    assert lib.mc_tiff_encode_slot_bytes(-1, ctypes.byref(out)) == -1
    assert lib.mc_tiff_encode_slot_bytes(10, None) == -1
    assert lib.mc_tiff_encode_slot_bytes(2**31, ctypes.byref(out)) == -2 and out.value == -7
    assert lib.mc_tiff_encode_slot_bytes(2**31 - 1, ctypes.byref(out)) == 0 and out.value >= closed_form(2**31 - 1)


# ------------------------------------------------------------------ the per-strip loop on the CPU, sanitized


def golden_strips(golden):
    """the pixel strips of every committed libtiff file with libtiff's own bytes for them -> [(name, rows, libtiff)]"""
    from test_tiff_host import fixture_strips

    out = []
    for name in NAMES:
        strips, rps, _, pixels = fixture_strips(golden, name)
        row_bytes = pixels.shape[2] * pixels.dtype.itemsize
        for frame, px in zip(strips, pixels):
            for theirs, rows in zip(frame, tr.strips_of(px.tobytes(), row_bytes, rps)):
                out.append((name, rows, theirs))
    return out


def test_strip_loop_on_the_host_under_sanitizers(golden, tmp_path):
    """csrc/tiff_lzw_encode.h -- the loop tiff_encode.hip compiles for the device -- is built for the host with
    -fsanitize=address,undefined into a program of its own and run as a child process on exactly-sized, poisoned
    buffers.  Its streams must equal tr.encode_strip's byte for byte, and tr.decode_strip must give the input back.
    Nothing sanitized is loaded into this process."""
    rng = np.random.default_rng(2)
    inputs = [b""] + [bytes([b]) for b in range(256)] + [bytes(n) for n in range(1, 1001)]
    inputs += [rng.poisson(1.0, n).astype(np.uint8).tobytes() for n in (63, 64, 65, 700, 7000)]
    noise = rng.integers(0, 256, 8192, dtype=np.uint8).tobytes()
    inputs += [noise, distinct_pairs(8000), bytes([3, 7] * 3000)]
    inputs += [rows for _, rows, _ in golden_strips(golden)]
    trace = []
    tr.decode_strip(tr.encode_strip(noise), len(noise), trace)
    assert {w for _, w, _ in trace} == {9, 10, 11, 12} and sum(c == tr.CLEAR for c, _, _ in trace) >= 2
    assert any(c == tr.CLEAR and n >= 4093 for c, _, n in trace)
    records = []
    for data in inputs:
        want = tr.encode_strip(data)
        assert tr.decode_strip(want, len(data)) == (data, "full")
        records.append(struct.pack("<2I", len(data), len(want)) + data + want)
    cases = tmp_path / "cases.bin"
    cases.write_bytes(b"".join(records))
    res = run_host_program("host_tiff_lzw_encode.cpp", tmp_path, cases)
    n_cases = int(re.search(r"(\d+) cases, 0 failures", res.stdout).group(1))
    assert n_cases == 6 * len(records) + 1


def test_libtiff_strips_compared_and_recorded(golden):
    """The rule's stream against libtiff's own bytes for the same rows.  Equality is NOT required -- libtiff's Clear
    heuristics are its own; DESIGN.md records the outcome -- but the rule's stream must decode to the rows, and so
    must libtiff's."""
    for name, rows, theirs in golden_strips(golden):
        ours = tr.encode_strip(rows)
        assert tr.decode_strip(ours, len(rows)) == (rows, "full")
        assert tr.decode_strip(theirs, len(rows))[0] == rows
        same = ours == theirs
        first = next((i for i, (a, b) in enumerate(zip(ours, theirs)) if a != b), min(len(ours), len(theirs)))
        print(f"LIBTIFF {name}: {len(rows)} bytes -> ours {len(ours)}, libtiff {len(theirs)}: "
              + ("equal" if same else f"first difference at byte {first}"))


# ------------------------------------------------------------------ the entry points' host checks


def test_entry_points_validate_on_the_host():
    """Fake device pointers and a null stream: every call below must answer before it touches or launches anything."""
    from torch_motion_correction_amd import _lib

    lib = _lib.load()
    p = [ctypes.c_void_p(0x100000 * (i + 1)) for i in range(4)]
    ARG, UNSUPPORTED = -1, -2
    slot = slot_bytes(5 * 8)

    def enc(src=p[0], n=2, h=8, row_bytes=8, rps=5, comp=5, slots=p[1], slot_bytes=slot, slots_bytes=4 * slot,
            produced=p[2]):
        return lib.mc_tiff_encode(src, n, h, row_bytes, rps, comp, slots, slot_bytes, slots_bytes, produced, None)

    for name in ("src", "slots", "produced"):
        assert enc(**{name: None}) == ARG, name
    assert enc(n=0) == ARG and enc(h=0) == ARG and enc(row_bytes=0) == ARG and enc(rps=0) == ARG and enc(rps=-2) == ARG
    assert enc(slot_bytes=0) == ARG and enc(slots_bytes=0) == ARG and enc(slots_bytes=-1) == ARG
    for comp in (1, 8, 32946, 7, 65001, 0, 2):
        assert enc(comp=comp) == UNSUPPORTED, comp
    assert enc(rps=9) == ARG  # more rows than the frame has
    assert enc(produced=ctypes.c_void_p(0x300004)) == ARG and enc(slots=ctypes.c_void_p(0x200008)) == ARG
    assert enc(slot_bytes=slot + 8, slots_bytes=4 * (slot + 8)) == ARG  # no multiple of 16
    assert enc(slot_bytes=slot - 16, slots_bytes=4 * slot) == ARG  # below the bound
    assert enc(slots_bytes=4 * slot - 1) == ARG  # 2 frames of 2 strips: short by one byte
    big = slot_bytes(2**31 - 2**15)
    assert enc(h=1 << 20, rps=1 << 16, row_bytes=1 << 15, slot_bytes=1 << 33, slots_bytes=1 << 40) == UNSUPPORTED
    assert enc(h=1 << 20, rps=(1 << 16) - 1, row_bytes=1 << 15, slot_bytes=big, slots_bytes=big) == ARG  # only short

    def pack(slots=p[0], slot_bytes=slot, offsets=p[1], produced=p[2], n=4, payload=p[3], payload_bytes=100):
        return lib.mc_tiff_pack(slots, slot_bytes, offsets, produced, n, payload, payload_bytes, None)

    for name in ("slots", "offsets", "produced", "payload"):
        assert pack(**{name: None}) == ARG, name
    assert pack(slot_bytes=0) == ARG and pack(n=0) == ARG and pack(payload_bytes=0) == ARG
    assert pack(offsets=ctypes.c_void_p(0x200004)) == ARG and pack(produced=ctypes.c_void_p(0x300004)) == ARG
    assert pack(n=2**31) == UNSUPPORTED


# ------------------------------------------------------------------ argument rules, devices refused


def test_argument_rules_hold_before_any_device_is_touched(mc, monkeypatch, tmp_path):
    from torch_motion_correction_amd import tiff

    def touched(*a, **k):
        raise AssertionError("a device was touched before the argument rules")

    monkeypatch.setattr(tiff, "require_gpu", touched)
    monkeypatch.setattr(tiff, "device_scope", touched)
    movie = torch.zeros(2, 8, 8, dtype=torch.uint8)
    path = tmp_path / "never.tif"

    def refuse(match, movie=movie, **kw):
        with pytest.raises(ValueError, match=match):
            mc.encode_tiff_raw(movie, **kw)
        with pytest.raises(ValueError, match=match):
            mc.write_tiff(path, movie, **kw)
        assert not path.exists()

    for bad in (np.zeros((2, 8, 8), np.uint8), torch.zeros(8, dtype=torch.uint8), torch.zeros(1, 2, 8, 8), b"abc"):
        refuse(r"\(t, h, w\) tensor", movie=bad)
    for bad in (torch.float16, torch.uint16, torch.int32, torch.float64, torch.int8, torch.int64, torch.bool):
        refuse("uint8, int16 or float32, got " + re.escape(str(bad)), movie=torch.zeros(2, 8, 8, dtype=bad))
    refuse("empty", movie=torch.zeros(0, 8, 8, dtype=torch.uint8))
    refuse("empty", movie=torch.zeros(2, 8, 0, dtype=torch.int16))
    for bad, word in ((8, "deflate"), (32946, "deflate"), (0, "got 0"), (True, "got True"), (None, "got None")):
        refuse(f"compression must be 5 .*{word}", compression=bad)
    for bad in (0, -1, 2.0, True, "3"):
        refuse("rows_per_strip must be an int >= 1", rows_per_strip=bad)
    with pytest.raises(ValueError, match="bigtiff must be"):
        mc.write_tiff(path, movie, compression=1, bigtiff=2)
    # the default strip: the most rows within 64 KB, at least one
    check = tiff._check_encode_args
    assert check(torch.zeros(1, 4092, 5760, dtype=torch.uint8).expand(40, -1, -1), None, 5)[3:5] == (11, 372)
    assert check(torch.zeros(1, 100, 5760, dtype=torch.float32), None, 5)[3] == 2
    assert check(torch.zeros(1, 3, 100000, dtype=torch.uint8), None, 5)[3] == 1
    assert check(torch.zeros(9, 20, dtype=torch.int16), None, 1) == (1, 9, 20, 9, 1, 40)
    assert check(movie, 100, 5)[3] == 8  # more rows than the frame has: the frame
    with pytest.raises(ValueError, match="2\\^31 bytes"):
        check(torch.zeros(1, 1, 1, dtype=torch.float32).expand(1, 4, 2**29), None, 5)


def test_file_plan_switches_to_bigtiff_when_offsets_need_it():
    from torch_motion_correction_amd import tiff

    small = [[100, 100, 50]] * 3
    big, strips, frames, size = tiff._plan_file(small, None)
    assert not big and strips[0] == [8, 108, 208] and strips[1][0] == 258
    assert all(o % 2 == 0 for f in frames for o in f) and frames[0][0] == 758
    assert tiff._plan_file(small, True)[0] and tiff._plan_file(small, True)[1][0][0] == 16
    huge = [[2**30] * 3] * 2  # 6 GB of strips
    assert tiff._plan_file(huge, None)[0] and tiff._plan_file(huge, True)[0]
    with pytest.raises(ValueError, match="do not fit the 32 bits of a classic TIFF"):
        tiff._plan_file(huge, False)
    edge = [[2**32 - 8 - 136]]  # header + strip + one IFD of 2 + 10 * 12 + 4 bytes: exactly 2^32 - 10
    assert not tiff._plan_file(edge, None)[0] and tiff._plan_file([[edge[0][0] + 12]], None)[0]


# ------------------------------------------------------------------ write_tiff, stored strips: no device


@pytest.mark.parametrize("bigtiff", [None, True])
@pytest.mark.parametrize("dtype,rps", [(torch.uint8, 5), (torch.int16, None), (torch.float32, 1)])
def test_write_tiff_stored_strips(mc, tmp_path, bigtiff, dtype, rps):
    g = torch.Generator().manual_seed(3)
    movie = (torch.randn(3, 12, 7, generator=g) * 50).to(dtype)
    path = tmp_path / "m.tif"
    mc.write_tiff(path, movie, rows_per_strip=rps, compression=1, bigtiff=bigtiff)
    raw = path.read_bytes()
    big, ifds = walk_ifds(raw)
    assert big is (bigtiff is True) and len(ifds) == 3
    want_rps = 12 if rps is None else rps
    size = movie.element_size()
    bits, fmt = {torch.uint8: (8, 1), torch.int16: (16, 2), torch.float32: (32, 3)}[dtype]
    long_type = 16 if big else 4
    frames = movie.numpy()
    at = 16 if big else 8
    for f, (ifd, tags) in enumerate(ifds):
        assert ifd % 2 == 0
        assert [t[0] for t in tags] == [256, 257, 258, 259, 262, 273, 277, 278, 279, 339]
        value = {t[0]: t for t in tags}
        spf = -(-12 // want_rps)
        assert [value[k][1:] for k in (256, 257, 258, 259, 262, 277, 278, 339)] == \
            [(4, 1, [7]), (4, 1, [12]), (3, 1, [bits]), (3, 1, [1]), (3, 1, [1]), (3, 1, [1]), (4, 1, [want_rps]),
             (3, 1, [fmt])]
        assert value[273][1:3] == (long_type, spf) and value[279][1:3] == (long_type, spf)
        for k, (o, n) in enumerate(zip(value[273][3], value[279][3])):
            rows = frames[f, k * want_rps:(k + 1) * want_rps].tobytes()
            assert o == at and n == len(rows) and raw[o:o + n] == rows  # in frame order, the strips are the rows
            at += n
    assert at == (16 if big else 8) + movie.numel() * size
    # read_tiff accepts it, and the strips it names are the movie
    got = mc.read_tiff(path)
    assert got.shape == (12, 7) and got.rows_per_strip == want_rps and got.compression == 1 and got.dtype == dtype
    data = bytes(got.data.numpy())
    assert b"".join(data[o:o + n] for fo, fn in zip(got.offsets, got.nbytes) for o, n in zip(fo, fn)) == \
        frames.tobytes()
    # a TiffMovie gives the same file; an (h, w) image is one frame; a non-contiguous view is made contiguous
    encoded = mc.encode_tiff_raw(movie, rows_per_strip=rps, compression=1)
    assert isinstance(encoded, mc.TiffMovie) and encoded.data.device.type == "cpu"
    assert encoded.offsets[1][0] == 12 * 7 * size and sum(sum(f) for f in encoded.nbytes) == movie.numel() * size
    other = tmp_path / "again.tif"
    mc.write_tiff(other, encoded, bigtiff=bigtiff)
    assert other.read_bytes() == raw
    mc.write_tiff(other, movie[1], rows_per_strip=rps, compression=1, bigtiff=bigtiff)
    one = mc.read_tiff(other)
    assert len(one.offsets) == 1 and bytes(one.data.numpy())[one.offsets[0][0]:][:12 * 7 * size] == frames[1].tobytes()
    view = movie.transpose(1, 2)
    mc.write_tiff(other, view, rows_per_strip=3, compression=1, bigtiff=bigtiff)
    back = mc.read_tiff(other)
    data = bytes(back.data.numpy())
    assert back.shape == (7, 12) and b"".join(data[o:o + n] for fo, fn in zip(back.offsets, back.nbytes)
                                              for o, n in zip(fo, fn)) == view.contiguous().numpy().tobytes()
