"""LZW-compressed TIFF movies (K3 / K2 counting detectors) decoded into raw movies on the device.

Counting detectors that do not write ``.eer`` write multi-page TIFF: one IFD per frame, strips of a few rows each,
LZW compression (TIFF compression 5), typically 8-bit counts; the gain reference (``.gain``) is a float32 TIFF of the
same container.  This module gives such a file a device route to the ``(t, h, w)`` tensor every raw route starts from:

  read_tiff        a pure-Python walk of the file's IFD chain -> ``TiffMovie`` (the bytes and each frame's strips)
  decode_tiff_raw  the strips decoded on the GPU, one wavefront per strip (mc_tiff_decode): the contiguous (t, h, w)
                   movie of the file's sample type
  encode_tiff_raw  the other direction: a raw movie encoded as LZW strips on the GPU, one wavefront per strip
                   (mc_tiff_encode, mc_tiff_pack) -> ``TiffMovie`` with the payload on the device
  write_tiff       that movie, or a tensor, written as a multi-page TIFF / BigTIFF file by host code

The decoded result is a raw movie for every ``*_raw*`` function, ``RawStatistics`` and the pipelines, as the output of
``render_eer_raw`` is.  The codec rule (TIFF 6.0 LZW: MSB-first codes, early change) is stated once, in
csrc/tiff_lzw.h, and is pinned to files written by libtiff (tests/golden/tiff_lzw_libtiff.npz).
"""

from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass

import torch

from ._files import _check_data, _check_fits_int16, _int, _positive_ints, read_file, require_tags, walk_ifds
from ._lib import check, device_scope, load, ptr, require_gpu, stream_ptr

# the file's sample type -> (bytes per sample, the dtype of the decoded movie)
_DTYPES = {torch.uint8: (1, torch.uint8), torch.int16: (2, torch.int16), torch.uint16: (2, torch.int16),
           torch.float32: (4, torch.float32)}
# (BitsPerSample, SampleFormat) -> the file's sample type
_SAMPLES = {(8, 1): torch.uint8, (16, 2): torch.int16, (16, 1): torch.uint16, (32, 3): torch.float32}

_TAG_NAMES = {256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression", 266: "FillOrder",
              273: "StripOffsets", 277: "SamplesPerPixel", 278: "RowsPerStrip", 279: "StripByteCounts",
              317: "Predictor", 322: "TileWidth", 323: "TileLength", 324: "TileOffsets", 325: "TileByteCounts",
              339: "SampleFormat"}
_ARRAY_TYPES = (3, 4, 16)  # StripOffsets / StripByteCounts: SHORT, LONG, LONG8, no BYTE


def _check_decode_args(data, offsets, nbytes, shape, rows_per_strip, compression, dtype):
    """Every argument rule of decode_tiff_raw -> (flat offsets, flat nbytes, t, strips per frame, h, w, rows per strip)
    as Python ints; ValueError otherwise."""
    _check_data(data)
    h, w = _positive_ints(shape, 2, f"shape must be the frames' (h, w), got {shape!r}")
    if dtype not in _DTYPES:
        raise ValueError(f"dtype must be torch.uint8, int16, uint16 (decoded to int16) or float32, got {dtype!r}")
    if isinstance(compression, bool) or compression not in (1, 5):
        raise ValueError(f"compression must be 5 (LZW) or 1 (none), got {compression!r}: deflate (8, 32946), JPEG "
                         "(7) and the EER codes (65000 - 65002, see read_eer) are not decoded")
    rps = min(_int(rows_per_strip, "rows_per_strip", 1), h)  # TIFF writers give 2^32 - 1 for "the whole frame"
    row_bytes = w * _DTYPES[dtype][0]
    if rps * row_bytes >= 2**31:
        raise ValueError(f"rows_per_strip={rps} of {row_bytes} bytes: strips that decode to 2^31 bytes and more are "
                         "not supported")
    spf = (h + rps - 1) // rps
    try:
        offsets = [[_int(o, "an offset", 0) for o in f] for f in offsets]
        nbytes = [[_int(n, "a byte count", 0) for n in f] for f in nbytes]
    except TypeError:
        raise ValueError("offsets and nbytes must be sequences, one per frame, of sequences of ints, one per "
                         "strip") from None
    if len(offsets) != len(nbytes) or not offsets:
        raise ValueError(f"offsets and nbytes must name the same frames, at least one: got {len(offsets)} and "
                         f"{len(nbytes)}")
    if len(offsets) * spf >= 2**31:
        raise ValueError(f"{len(offsets)} frames of {spf} strips: 2^31 strips and more are not supported")
    total = int(data.numel())
    for i, (fo, fn) in enumerate(zip(offsets, nbytes)):
        if len(fo) != spf or len(fn) != spf:
            raise ValueError(f"frame {i}: {len(fo)} offsets and {len(fn)} byte counts, but {h} rows in strips of "
                             f"{rps} are {spf} strips")
        for k, (o, n) in enumerate(zip(fo, fn)):
            if o + n > total:
                raise ValueError(f"frame {i}, strip {k}: offset {o}, {n} bytes leaves the {total} bytes of data")
    flat_o = [o for f in offsets for o in f]
    flat_n = [n for f in nbytes for n in f]
    return flat_o, flat_n, len(offsets), spf, h, w, rps


def _decode_strips(data, flat_o, flat_n, t, spf, h, row_bytes, rps, compression, device, out=None):
    """The checked arguments decoded -> (the (t * h * row_bytes,) uint8 output, the per-strip bytes produced), both on
    the device.  `out`: a buffer to decode into (the tests' guarded buffers)."""
    dev = require_gpu(device if device is not None else data.device)
    n = t * spf
    with device_scope(dev):
        buf = data.detach().to(dev).contiguous()
        if buf.numel() == 0:  # strips without bytes: a pointer the library can take
            buf = torch.zeros(8, dtype=torch.uint8, device=dev)
        if out is None:
            out = torch.empty(t * h * row_bytes, dtype=torch.uint8, device=dev)
        assert out.dtype == torch.uint8 and out.numel() == t * h * row_bytes and out.device == dev
        scratch = torch.empty(2 * n, dtype=torch.int64, device=dev)
        produced = torch.empty(n, dtype=torch.int32, device=dev)
        off_c, nb_c = (C.c_int64 * n)(*flat_o), (C.c_int64 * n)(*flat_n)
        check(load().mc_tiff_decode(ptr(buf), int(data.numel()), off_c, nb_c, t, spf, h, row_bytes, rps, compression,
                                    ptr(out), ptr(produced), ptr(scratch), 8 * scratch.numel(), stream_ptr(dev)),
              "mc_tiff_decode")
    return out, produced


def _expected(spf, h, row_bytes, rps):
    """the bytes of each strip of one frame"""
    return [min(rps, h - k * rps) * row_bytes for k in range(spf)]


def decode_tiff_raw(data, offsets, nbytes, shape, rows_per_strip, compression=5, dtype=torch.uint8, device=None):
    """TIFF strips decoded into a raw movie: the contiguous ``(t, h, w)`` tensor on the GPU whose frame ``f`` is the
    strips ``offsets[f]`` put below one another, ``rows_per_strip`` rows each (the last strip of a frame holds the
    rest).

    ``data``: a 1-D uint8 tensor (CPU or GPU) that holds the strips anywhere in it, in any order, with anything
    between them -- it may be the whole file.  ``offsets`` / ``nbytes``: one list per frame of one int per strip, the
    strip's first byte and length in ``data``; every frame has ``ceil(h / rows_per_strip)`` strips (a
    ``rows_per_strip`` above ``h`` means ``h``).  ``shape``: the frames' ``(h, w)``.  ``compression``: 5, TIFF 6.0
    LZW (csrc/tiff_lzw.h states the rule), or 1, stored rows.  ``dtype`` names the file's samples: ``torch.uint8``,
    ``torch.int16``, ``torch.float32`` (little-endian), or ``torch.uint16`` for unsigned 16-bit files, which are
    returned as ``int16`` -- the raw routes' 16-bit type -- and raise ValueError if a sample is 32768 or more.

    Exact: the decoder moves bytes.  A strip that gives fewer bytes than its rows need (cut short, a malformed code,
    an early end-of-information) raises ValueError naming the first such frame and strip -- from the one
    device-to-host read of the per-strip byte counts; bytes a strip holds beyond its rows are ignored, as libtiff
    ignores them.  Every other argument rule, a strip outside ``data`` included, is a ValueError raised before any
    device is touched.  The kernel reads no byte outside a strip and writes no byte outside that strip's rows,
    whatever its bits say.

    ``device``: the GPU to decode on (None: the device of ``data``, the current GPU for a CPU tensor)."""
    flat_o, flat_n, t, spf, h, w, rps = _check_decode_args(data, offsets, nbytes, shape, rows_per_strip, compression,
                                                           dtype)
    size, out_dtype = _DTYPES[dtype]
    out, produced = _decode_strips(data, flat_o, flat_n, t, spf, h, w * size, rps, compression, device)
    got = produced.cpu().tolist()
    want = _expected(spf, h, w * size, rps)
    for s, g in enumerate(got):
        if g != want[s % spf]:
            raise ValueError(f"frame {s // spf}, strip {s % spf}: its {flat_n[s]} bytes decode to {g} of the "
                             f"{want[s % spf]} bytes of its rows: not a well-formed "
                             f"{'LZW' if compression == 5 else 'stored'} strip")
    movie = out.view(out_dtype).view(t, h, w)
    if dtype == torch.uint16:
        _check_fits_int16(movie)
    return movie


@dataclass
class TiffMovie:
    """A TIFF movie as ``read_tiff`` found it: ``data`` (1-D uint8, the whole file), ``offsets`` / ``nbytes`` (one
    list of ints per frame, one int per strip), ``shape`` (h, w), ``rows_per_strip``, ``compression`` (1 or 5) and
    ``dtype`` (the file's sample type: torch.uint8, int16, uint16 or float32)."""

    data: torch.Tensor
    offsets: list
    nbytes: list
    shape: tuple
    rows_per_strip: int
    compression: int
    dtype: torch.dtype

    def decode(self, device=None):
        """``decode_tiff_raw`` of this movie."""
        return decode_tiff_raw(self.data, self.offsets, self.nbytes, self.shape, self.rows_per_strip,
                               compression=self.compression, dtype=self.dtype, device=device)


def read_tiff(path):
    """A TIFF movie -> ``TiffMovie``: a walk of the TIFF (magic 42) or BigTIFF (magic 43) IFD chain, in either byte
    order, in plain Python; no decoder is involved.  Every IFD is one frame of one or more strips and must give
    ImageWidth, ImageLength, Compression, StripOffsets and StripByteCounts (arrays of SHORT, LONG or LONG8, inline or
    out of line).  Absent tags mean BitsPerSample 1 (refused), SamplesPerPixel 1, RowsPerStrip = ImageLength,
    SampleFormat 1, Predictor 1, FillOrder 1.

    Accepted samples: 8-bit unsigned (uint8), 16-bit signed (int16), 16-bit unsigned (uint16: decoded to int16,
    refused at decode time if a sample is 32768 or more) and 32-bit float (float32, the gain file); multi-byte
    samples need a little-endian (``II``) file.  Compression 5 (LZW) and 1 (none).  Everything else -- deflate, JPEG,
    the EER codes, Predictor 2 or 3, FillOrder 2, more than one sample per pixel, tiles, other bit depths, frames that
    differ from the first, a strip count other than ceil(h / RowsPerStrip), a strip or an IFD that leaves the file, a
    looping chain, an empty file -- raises ValueError with the frame and the tag named.

    The Orientation tag is ignored: rows are returned in stored order."""
    raw, size, data = read_file(path)

    def fail(msg):
        raise ValueError(f"{path}: {msg}")

    if size == 0:
        fail("the file is empty")
    offsets, nbytes, first = [], [], None
    for i, found in enumerate(walk_ifds(raw, size, _TAG_NAMES, fail)):
        for tag in range(322, 326):
            if tag in found:
                fail(f"frame {i}: {_TAG_NAMES[tag]} ({tag}): tiled TIFF is not supported, only strips")
        require_tags(found, _TAG_NAMES, i, fail)
        tags = {}
        for tag, (typ, values) in found.items():  # Orientation is not among them: rows stay in stored order
            if tag in (273, 279):
                if typ not in _ARRAY_TYPES:
                    fail(f"frame {i}: {_TAG_NAMES[tag]} has TIFF type {typ}, not one of {sorted(_ARRAY_TYPES)} "
                         "(unsigned integers)")
                tags[tag] = values
            elif len(values) != 1:
                fail(f"frame {i}: {_TAG_NAMES[tag]} has {len(values)} values"
                     + ("; SamplesPerPixel other than 1 is not supported" if tag in (258, 339) else ""))
            else:
                tags[tag] = values[0]
        h, w, comp = tags[257], tags[256], tags[259]
        if h < 1 or w < 1:
            fail(f"frame {i}: ImageLength x ImageWidth {(h, w)} is empty")
        if comp not in (1, 5):
            fail(f"frame {i}: Compression {comp} is not supported: 5 (LZW) and 1 (none) are; 8 / 32946 (deflate), 7 "
                 "(JPEG) and 65000 - 65002 (EER, see read_eer) are not")
        if tags.get(317, 1) != 1:
            fail(f"frame {i}: Predictor {tags[317]} is not supported (only 1, none)")
        if tags.get(266, 1) != 1:
            fail(f"frame {i}: FillOrder {tags[266]} is not supported (only 1, MSB first)")
        if tags.get(277, 1) != 1:
            fail(f"frame {i}: SamplesPerPixel {tags[277]} is not supported (only 1)")
        bits, fmt = tags.get(258, 1), tags.get(339, 1)
        if (bits, fmt) not in _SAMPLES:
            fail(f"frame {i}: BitsPerSample {bits} with SampleFormat {fmt} is not supported: 8-bit unsigned, 16-bit "
                 "signed or unsigned and 32-bit float samples are")
        if bits > 8 and raw[:2] == b"MM":
            fail(f"frame {i}: BitsPerSample {bits} in a big-endian (MM) file is not supported")
        rps = min(tags.get(278, h), h)
        if rps < 1:
            fail(f"frame {i}: RowsPerStrip {tags[278]}")
        this = (h, w, comp, _SAMPLES[bits, fmt], rps)
        if first is None:
            first = this
        else:
            for a, b, name in zip(this, first, ("ImageLength", "ImageWidth", "Compression",
                                                "BitsPerSample / SampleFormat", "RowsPerStrip")):
                if a != b:
                    fail(f"frame {i}: {name} {a} differs from the first frame's {b}")
        spf = (h + rps - 1) // rps
        if len(tags[273]) != spf or len(tags[279]) != spf:
            fail(f"frame {i}: StripOffsets has {len(tags[273])} and StripByteCounts {len(tags[279])} values, but "
                 f"{h} rows in strips of {rps} are {spf} strips")
        for k, (o, n) in enumerate(zip(tags[273], tags[279])):
            if o + n > size:
                fail(f"frame {i}, strip {k}: StripOffsets + StripByteCounts = {o + n} leaves the file of {size} "
                     "bytes")
        offsets.append(tags[273])
        nbytes.append(tags[279])
    h, w, comp, dtype, rps = first
    return TiffMovie(data=data, offsets=offsets, nbytes=nbytes, shape=(h, w), rows_per_strip=rps, compression=comp,
                     dtype=dtype)


# ------------------------------------------------------------------ raw movies -> LZW strips -> TIFF / BigTIFF files

# the sample type -> (BitsPerSample, SampleFormat) of the file
_FILE_SAMPLES = {dtype: key for key, dtype in _SAMPLES.items()}
_ENCODE_DTYPES = (torch.uint8, torch.int16, torch.float32)
_STRIP_TARGET = 65536  # rows_per_strip=None: the largest strip of at most this many bytes, as libtiff cuts them


def _check_encode_args(movie, rows_per_strip, compression):
    """Every argument rule of encode_tiff_raw -> (t, h, w, rows per strip, strips per frame, row bytes) as Python
    ints; ValueError otherwise."""
    if not isinstance(movie, torch.Tensor) or movie.dim() not in (2, 3):
        raise ValueError("movie must be a (t, h, w) tensor, or (h, w) for one image, got "
                         f"{type(movie).__name__} {tuple(getattr(movie, 'shape', ()))}")
    if movie.dtype not in _ENCODE_DTYPES:
        raise ValueError(f"movie must be torch.uint8, int16 or float32, got {movie.dtype}: the raw routes' types and "
                         "the gain's are written, nothing is converted")
    t, h, w = (1, *movie.shape) if movie.dim() == 2 else movie.shape
    if t < 1 or h < 1 or w < 1:
        raise ValueError(f"movie is empty: {tuple(movie.shape)}")
    if isinstance(compression, bool) or compression not in (1, 5):
        raise ValueError(f"compression must be 5 (LZW) or 1 (none), got {compression!r}: deflate (8, 32946), "
                         "Predictor 2 and tiles are not written")
    row_bytes = w * _DTYPES[movie.dtype][0]
    if rows_per_strip is None:
        rps = max(1, min(h, _STRIP_TARGET // row_bytes))
    else:
        rps = min(_int(rows_per_strip, "rows_per_strip", 1), h)
    if rps * row_bytes >= 2**31:
        raise ValueError(f"rows_per_strip={rps} of {row_bytes} bytes: strips of 2^31 bytes and more are not supported")
    spf = (h + rps - 1) // rps
    if t * spf >= 2**31:
        raise ValueError(f"{t} frames of {spf} strips: 2^31 strips and more are not supported")
    return t, h, w, rps, spf, row_bytes


def _slot_bytes(strip_bytes):
    """mc_tiff_encode_slot_bytes: the bound, a multiple of 16, on the stream of a strip of `strip_bytes` bytes"""
    out = C.c_int64(0)
    check(load().mc_tiff_encode_slot_bytes(strip_bytes, C.byref(out)), "mc_tiff_encode_slot_bytes")
    return out.value


def _encode_strips(src, t, spf, h, row_bytes, rps, dev, slots=None):
    """The movie's bytes (1-D uint8 on `dev`) encoded -> (slots, bytes per slot, the per-strip byte counts as int64),
    on the device.  `slots`: a 16-byte-aligned buffer of t * spf slots to encode into (the tests' guarded buffers)."""
    n, slot = t * spf, _slot_bytes(rps * row_bytes)
    with device_scope(dev):
        if slots is None:
            slots = torch.empty(n * slot, dtype=torch.uint8, device=dev)
        assert slots.dtype == torch.uint8 and slots.numel() == n * slot and slots.device == dev
        produced = torch.empty(n, dtype=torch.int64, device=dev)
        check(load().mc_tiff_encode(ptr(src), t, h, row_bytes, rps, 5, ptr(slots), slot, slots.numel(), ptr(produced),
                                    stream_ptr(dev)), "mc_tiff_encode")
    return slots, slot, produced


def _pack_strips(slots, slot, produced, total, dev, payload=None):
    """Every slot's produced bytes moved to their place in one payload of `total` bytes, at the exclusive scan of
    `produced`, which runs on the device -> the payload.  `payload`: a buffer to pack into."""
    with device_scope(dev):
        offsets = torch.cumsum(produced, 0) - produced
        if payload is None:
            payload = torch.empty(total, dtype=torch.uint8, device=dev)
        assert payload.dtype == torch.uint8 and payload.numel() == total and payload.device == dev
        check(load().mc_tiff_pack(ptr(slots), slot, ptr(offsets), ptr(produced), produced.numel(), ptr(payload), total,
                                  stream_ptr(dev)), "mc_tiff_pack")
    return payload


def encode_tiff_raw(movie, rows_per_strip=None, compression=5, device=None):
    """A raw movie encoded as TIFF strips -> ``TiffMovie``: the inverse of ``decode_tiff_raw``, and what
    ``write_tiff`` puts into a file.

    ``movie``: ``(t, h, w)``, or ``(h, w)`` for one image such as a gain; ``torch.uint8``, ``int16`` or ``float32``,
    CPU or GPU, any strides (it is made contiguous).  ``rows_per_strip``: the rows of a strip (the last strip of a
    frame holds the rest; a value above ``h`` means ``h``); None picks the most rows whose strip is at most 64 KB, at
    least one.  ``compression``: 5, TIFF 6.0 LZW, one wavefront per strip on the GPU (mc_tiff_encode, then
    mc_tiff_pack), or 1, stored rows, which needs no kernel: the payload is the movie's bytes, left where the movie
    is unless ``device`` says otherwise.

    The returned movie has ``data`` = the strips one after another in frame order -- on the GPU for compression 5 --
    ``offsets`` / ``nbytes`` as lists of ints per frame, ``shape``, ``rows_per_strip``, ``compression`` and ``dtype``;
    ``.decode()`` gives the movie back bit for bit.  The encoder is deterministic: a leading Clear, greedy longest
    match, Clear once the decoder's next code reaches 4093, EOI (csrc/tiff_lzw_encode.h states the rule; every
    strip's bytes equal tests/tiff_reference.py::encode_strip's).  There is one device-to-host read, of the
    per-strip sizes.  Every argument rule is a ValueError raised before any device is touched.

    ``device``: the GPU to encode on (None: the device of ``movie``, the current GPU for a CPU tensor)."""
    t, h, w, rps, spf, row_bytes = _check_encode_args(movie, rows_per_strip, compression)
    if compression == 1:
        data = movie.detach()
        if device is not None:
            data = data.to(require_gpu(device))
        data = data.contiguous().view(torch.uint8).reshape(-1)
        sizes = _expected(spf, h, row_bytes, rps) * t
    else:
        dev = require_gpu(device if device is not None else movie.device)
        with device_scope(dev):
            src = movie.detach().to(dev).contiguous().view(torch.uint8).reshape(-1)
        slots, slot, produced = _encode_strips(src, t, spf, h, row_bytes, rps, dev)
        sizes = produced.cpu().tolist()
        data = _pack_strips(slots, slot, produced, sum(sizes), dev)
    offsets, at = [], 0
    for n in sizes:
        offsets.append(at)
        at += n
    return TiffMovie(data=data, offsets=[offsets[f * spf:(f + 1) * spf] for f in range(t)],
                     nbytes=[sizes[f * spf:(f + 1) * spf] for f in range(t)], shape=(h, w), rows_per_strip=rps,
                     compression=compression, dtype=movie.dtype)


def _plan_file(nbytes, bigtiff):
    """Where everything of a file with these strip sizes (one list per frame) goes: the header, the strips in frame
    order, then per frame its out-of-line arrays and its IFD, each at an even offset -> (big, per frame the strip
    offsets, per frame (StripOffsets array, StripByteCounts array, IFD) offsets with None for an inline array, the
    file's size).  bigtiff None: BigTIFF exactly when an offset of the classic layout does not fit 32 bits."""
    if bigtiff not in (None, True, False):
        raise ValueError(f"bigtiff must be None, True or False, got {bigtiff!r}")

    def plan(big):
        word, entry, head = (8, 20, 8) if big else (4, 12, 2)
        at = 16 if big else 8
        strips = []
        for f in nbytes:
            strips.append([])
            for n in f:
                strips[-1].append(at)
                at += n
        frames = []
        for f in nbytes:
            arrays = []
            for _ in range(2):
                if len(f) * word > word:  # more than one value: out of line
                    at += at & 1
                    arrays.append(at)
                    at += len(f) * word
                else:
                    arrays.append(None)
            at += at & 1
            frames.append((arrays[0], arrays[1], at))
            at += head + 10 * entry + word
        return strips, frames, at

    strips, frames, size = plan(False)
    fits = size <= 2**32 and all(n < 2**32 for f in nbytes for n in f)
    if bigtiff is False and not fits:
        raise ValueError(f"the file has {size} bytes: its offsets do not fit the 32 bits of a classic TIFF; pass "
                         "bigtiff=None or True")
    big = bool(bigtiff) or not fits
    return (big, *(plan(True) if big else (strips, frames, size)))


def write_tiff(path, movie, rows_per_strip=None, compression=5, bigtiff=None, device=None):
    """A raw movie written as a multi-page TIFF or BigTIFF file, one IFD per frame, in strips.

    ``movie``: a tensor -- ``encode_tiff_raw(movie, rows_per_strip, compression, device)`` runs first -- or a
    ``TiffMovie`` such as that function returns, whose own rows per strip and compression are written
    (``rows_per_strip``, ``compression`` and ``device`` are then not looked at).  Host code writes the little-endian
    file: the header, the strips in frame order, then per frame its StripOffsets / StripByteCounts arrays (when they
    hold more than one value) and its IFD, each at an even offset.  Every IFD holds, in ascending order, ImageWidth,
    ImageLength, BitsPerSample, Compression, PhotometricInterpretation 1, StripOffsets, SamplesPerPixel 1,
    RowsPerStrip, StripByteCounts and SampleFormat (1 unsigned, 2 signed, 3 float); no resolution tags.

    ``bigtiff``: None writes BigTIFF (magic 43, LONG8 offsets) exactly when an offset does not fit 32 bits, True
    always, False never -- a file that needs it is then a ValueError, raised before anything is written.
    ``read_tiff`` reads what this writes."""
    if not isinstance(movie, TiffMovie):
        movie = encode_tiff_raw(movie, rows_per_strip=rows_per_strip, compression=compression, device=device)
    if movie.dtype not in _FILE_SAMPLES or movie.compression not in (1, 5):
        raise ValueError(f"a TiffMovie of {movie.dtype}, compression {movie.compression} cannot be written")
    h, w = movie.shape
    bits, fmt = _FILE_SAMPLES[movie.dtype]
    big, strips, frames, size = _plan_file(movie.nbytes, bigtiff)
    bytes_ = memoryview(movie.data.detach().cpu().contiguous().numpy())
    word, long_type = ("Q", 16) if big else ("I", 4)
    with open(path, "wb") as fh:
        first = frames[0][2] if frames else 0
        fh.write(struct.pack("<2sHHHQ", b"II", 43, 8, 0, first) if big else struct.pack("<2sHI", b"II", 42, first))
        at = 16 if big else 8
        # the strips in frame order; strips that follow one another in `data` go out in one write
        runs = []
        for fo, fn in zip(movie.offsets, movie.nbytes):
            for o, n in zip(fo, fn):
                if runs and runs[-1][1] == o:
                    runs[-1][1] = o + n
                else:
                    runs.append([o, o + n])
                at += n
        for a, b in runs:
            fh.write(bytes_[a:b])

        def pad_to(where):
            nonlocal at
            fh.write(bytes(where - at))
            at = where

        def put(blob):
            nonlocal at
            fh.write(blob)
            at += len(blob)

        for i, (fn, so, (arr_o, arr_n, ifd)) in enumerate(zip(movie.nbytes, strips, frames)):
            if arr_o is not None:
                pad_to(arr_o)
                put(struct.pack(f"<{len(so)}{word}", *so))
                pad_to(arr_n)
                put(struct.pack(f"<{len(fn)}{word}", *fn))
            pad_to(ifd)
            entries = [(256, 4, 1, w), (257, 4, 1, h), (258, 3, 1, bits), (259, 3, 1, movie.compression),
                       (262, 3, 1, 1), (273, long_type, len(so), so[0] if arr_o is None else arr_o), (277, 3, 1, 1),
                       (278, 4, 1, movie.rows_per_strip), (279, long_type, len(fn), fn[0] if arr_n is None else arr_n),
                       (339, 3, 1, fmt)]
            blob = struct.pack("<Q" if big else "<H", len(entries))
            for tag, typ, count, value in entries:  # a value smaller than its field sits at the field's low end
                blob += struct.pack("<HHQQ" if big else "<HHII", tag, typ, count, value)
            blob += struct.pack("<" + word, frames[i + 1][2] if i + 1 < len(frames) else 0)
            put(blob)
        assert at == size
