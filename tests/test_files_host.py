"""What eer.py, tiff.py and mrc.py share (torch_motion_correction_amd/_files.py), without a GPU: the one IFD walker on
TIFF and BigTIFF files of both byte orders written by tests/tiff_files.py, against that module's independent struct
walk; the chains and arrays it must refuse; read_file's one copy of the file; the argument rules' messages; that the
module touches no device; and that read_eer and read_tiff get their IFDs from the walker and from nowhere else."""

import re
import struct

import numpy as np
import pytest
import torch

import eer_reference as er
import tiff_files
import tiff_reference as tr
from torch_motion_correction_amd import _files, eer, mrc, tiff

NAMES = {256: "ImageWidth", 257: "ImageLength", 259: "Compression", 273: "StripOffsets", 279: "StripByteCounts"}
TAGS = {256: (4, 1, 20), 257: (3, 1, 37), 259: (3, 1, 5), 262: (3, 1, 1)}  # 262 is not in NAMES


class Refused(Exception):
    pass


def fail(msg):
    raise Refused("here: " + msg)


def strips_of(seed, frames, per_frame):
    rng = np.random.default_rng(seed)
    return [[bytes(rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8)) for _ in range(per_frame)]
            for _ in range(frames)]


def walked(path):
    raw = path.read_bytes()
    return list(_files.walk_ifds(raw, len(raw), NAMES, fail))


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("byte_order", ["<", ">"])
@pytest.mark.parametrize("per_frame,types", [(1, (4, 4)), (2, (3, 4)), (5, (3, 16)), (3, (16, 3))])
def test_walker_against_the_independent_walk(tmp_path, big, byte_order, per_frame, types):
    """Inline and out-of-line arrays of every integer type, IFDs between strips, a chain that jumps back and forth."""
    strips = strips_of(per_frame, 4, per_frame)
    path = tmp_path / "f.tif"
    offsets, nbytes = tiff_files.write_tiff(path, strips, TAGS, big=big, byte_order=byte_order, order=[2, 0, 3, 1],
                                            array_types=types, overrides={1: {257: (1, 1, 37)}})
    raw = path.read_bytes()
    for fo, fs in zip(offsets, strips):
        assert all(o % 2 == 1 and raw[o:o + len(s)] == s for o, s in zip(fo, fs))
    is_big, ifds = tiff_files.walk_ifds(raw)
    assert is_big is big and len(ifds) == 4
    at = [ifd for ifd, _ in ifds]
    assert at != sorted(at) and min(at) < max(o for fo in offsets for o in fo)  # the chain jumps; IFDs between strips
    got = walked(path)
    assert len(got) == 4
    for f, (found, (_, entries)) in enumerate(zip(got, ifds)):
        assert [e[0] for e in entries] == [256, 257, 259, 262, 273, 279]
        assert found == {tag: (typ, values) for tag, typ, _, values in entries if tag in NAMES}
        assert found[273] == (types[0], offsets[f]) and found[279] == (types[1], nbytes[f])
        assert found[257] == ((1 if f == 1 else 3), [37]) and 262 not in found


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("byte_order", ["<", ">"])
def test_walker_refusals(tmp_path, big, byte_order):
    strips = strips_of(7, 3, 3)
    path = tmp_path / "bad.tif"
    kw = dict(big=big, byte_order=byte_order)

    def refuse(match, **more):
        tiff_files.write_tiff(path, strips, TAGS, **kw, **more)
        with pytest.raises(Refused, match=match):
            walked(path)

    refuse("here: frame 3: the IFD chain loops", loop=True)
    refuse("here: frame 1: StripByteCounts: its 3 values at offset 10000000 leave the file of",
           overrides={1: {279: (16, 3, 10**7)}})
    refuse("here: frame 2: StripOffsets: its 900 values at offset 64 leave the file",
           overrides={2: {273: (4, 900, 64)}})
    refuse("here: frame 0: ImageWidth has TIFF type 5, not one of", overrides={0: {256: (5, 1, 64)}})
    refuse("here: frame 1: Compression has no value", overrides={1: {259: (3, 0, 5)}})
    # an IFD past the end of the file: the first, and one later in the chain; an IFD cut by the end of the file
    tiff_files.write_tiff(path, strips, TAGS, **kw)
    good = path.read_bytes()
    word = byte_order + ("Q" if big else "I")
    raw = bytearray(good)
    struct.pack_into(word, raw, 8 if big else 4, len(raw) + 10)
    with pytest.raises(Refused, match="here: frame 0: its IFD lies outside the file"):
        list(_files.walk_ifds(raw, len(raw), NAMES, fail))
    first = tiff_files.walk_ifds(good)[1][0][0]
    raw = bytearray(good)
    struct.pack_into(word, raw, first + (8 + 20 * 6 if big else 2 + 12 * 6), len(raw) - 1)
    with pytest.raises(Refused, match="here: frame 1: its IFD lies outside the file"):
        list(_files.walk_ifds(raw, len(raw), NAMES, fail))
    last = max(ifd for ifd, _ in tiff_files.walk_ifds(good)[1])
    with pytest.raises(Refused, match="its IFD lies outside the file"):
        list(_files.walk_ifds(good, last + 20, NAMES, fail))
    # the header
    for raw, match in ((b"", "not a TIFF"), (b"II*", "not a TIFF"), (b"PK\x03\x04" + bytes(12), "not a TIFF"),
                       (b"II" + (44).to_bytes(2, "little") + bytes(12), "magic 44"),
                       (b"MM\x00\x2b\x00\x04\x00\x00" + bytes(8), "offset size other than 8"),
                       (b"II*\x00" + bytes(4), "here: the file holds no frame")):
        with pytest.raises(Refused, match=match):
            list(_files.walk_ifds(raw, len(raw), NAMES, fail))


def test_read_file_shares_one_copy(tmp_path):
    path = tmp_path / "bytes.bin"
    path.write_bytes(bytes(range(200)))
    raw, size, data = _files.read_file(path)
    assert isinstance(raw, bytearray) and size == len(raw) == 200 and raw == bytes(range(200))
    assert data.dtype == torch.uint8 and data.shape == (200,) and data.tolist() == list(range(200))
    raw[5] = 77
    assert int(data[5]) == 77
    data[9] = 88
    assert raw[9] == 88
    path.write_bytes(b"")
    raw, size, data = _files.read_file(str(path))
    assert raw == b"" and size == 0 and data.dtype == torch.uint8 and data.shape == (0,)


def test_readers_hand_out_the_shared_buffer(tmp_path, monkeypatch):
    """read_eer, read_tiff and read_mrc return read_file's tensor itself: there is no second copy of the file."""
    import mrc_reference as mr

    handed = []

    def recording(path):
        handed.append(_files.read_file(path))
        return handed[-1]

    for module in (eer, tiff, mrc):
        monkeypatch.setattr(module, "read_file", recording)
    strips = strips_of(1, 2, 1)
    er.write_tiff(tmp_path / "m.eer", [f[0] for f in strips], (4, 8))
    tr.write_tiff(tmp_path / "m.tif", strips, (4, 8), 4)
    mr.write_mrc(tmp_path / "m.mrc", np.zeros((2, 3, 4), np.int16), 1)
    for read, name in ((eer.read_eer, "m.eer"), (tiff.read_tiff, "m.tif"), (mrc.read_mrc, "m.mrc")):
        movie = read(tmp_path / name)
        raw, size, data = handed[-1]
        assert movie.data is data and size == (tmp_path / name).stat().st_size
        raw[0] ^= 0xff
        assert int(movie.data[0]) == raw[0]
    assert len(handed) == 3


def test_no_device_helper_is_in_reach():
    for name in ("require_gpu", "device_scope", "load", "ptr", "stream_ptr", "check"):
        assert not hasattr(_files, name), name
    for module in (eer, tiff, mrc):  # one definition of each rule
        assert module._int is _files._int and module._check_data is _files._check_data
    assert tiff._check_fits_int16 is mrc._check_fits_int16 is _files._check_fits_int16
    assert not hasattr(eer, "_INT_TYPES") and not hasattr(tiff, "_INT_TYPES")


def test_the_integer_rules_and_their_messages():
    assert _files._int(5, "n", 1) == 5 and _files._int(np.int64(0), "n", 0) == 0 and _files._int(-9, "k") == -9
    for bad in (0, -1, 2.0, None, True, "3"):
        with pytest.raises(ValueError, match="^group must be an int >= 1, got " + re.escape(repr(bad)) + "$"):
            _files._int(bad, "group", 1)
    for bad in (1.0, None, "1", False):
        with pytest.raises(ValueError, match="^rot90 must be an int, got " + re.escape(repr(bad)) + "$"):
            _files._int(bad, "rot90")
    assert _files._positive_ints((3, np.int32(4)), 2, "no") == [3, 4]
    assert _files._positive_ints([2, 3, 4], 3, "no") == [2, 3, 4]
    for bad, n in (((8,), 2), ((8, 8, 8), 2), ((0, 8), 2), ((8, -1), 2), (8, 2), ((8.0, 8), 2), ((True, 8), 2),
                   (None, 3), ((2, 3), 3)):
        with pytest.raises(ValueError, match="^the caller's words$"):
            _files._positive_ints(bad, n, "the caller's words")
    _files._check_data(torch.zeros(3, dtype=torch.uint8))
    for bad in (np.zeros(3, np.uint8), torch.zeros(3, dtype=torch.int8), torch.zeros(2, 2, dtype=torch.uint8), b"abc"):
        with pytest.raises(ValueError, match="data must be a 1-D uint8 tensor, got"):
            _files._check_data(bad)
    _files._check_fits_int16(torch.tensor([0, 32767], dtype=torch.int16))
    with pytest.raises(ValueError, match="an unsigned 16-bit sample is 32768 or more"):
        _files._check_fits_int16(torch.tensor([0, -32768], dtype=torch.int16))


@pytest.mark.parametrize("module,reader", [(eer, "read_eer"), (tiff, "read_tiff")])
def test_readers_get_their_ifds_from_the_shared_walker(tmp_path, monkeypatch, module, reader):
    """The reader calls _files.walk_ifds with the file's bytes, its own tag names and a `fail` that names the path;
    and what it returns is made of what the walker yields -- IFDs the file does not hold included."""
    assert module.walk_ifds is _files.walk_ifds
    strips = strips_of(2, 3, 1)
    path = tmp_path / "movie"
    if module is eer:
        offsets, nbytes = er.write_tiff(path, [f[0] for f in strips], (4, 8))
    else:
        offsets, nbytes = tr.write_tiff(path, strips, (4, 8), 4, compression=1)
    calls = []

    def recording(raw, size, names, fail):
        calls.append((bytes(raw), size, names, fail))
        return _files.walk_ifds(raw, size, names, fail)

    monkeypatch.setattr(module, "walk_ifds", recording)
    movie = getattr(module, reader)(path)
    assert movie.offsets == offsets and movie.nbytes == nbytes and movie.shape == (4, 8)
    (raw, size, names, reader_fail), = calls
    assert raw == path.read_bytes() and size == len(raw) and names is module._TAG_NAMES
    with pytest.raises(ValueError, match="^" + re.escape(str(path)) + ": words$"):
        reader_fail("words")

    comp = 65001 if module is eer else 1
    made_up = {256: (4, [12]), 257: (4, [5]), 259: (3, [comp]), 258: (3, [8]), 273: (4, [1]), 279: (4, [2])}
    monkeypatch.setattr(module, "walk_ifds", lambda *a: iter([made_up, made_up]))
    movie = getattr(module, reader)(path)
    assert movie.shape == (5, 12) and len(movie.offsets) == 2
    assert movie.offsets == ([1, 1] if module is eer else [[1], [1]])
    monkeypatch.setattr(module, "walk_ifds", lambda *a: iter([{**made_up, 256: (4, [12, 13])}]))
    with pytest.raises(ValueError, match="frame 0: ImageWidth has 2 values"):
        getattr(module, reader)(path)
