"""MRC / MRCS movies and gain references decoded into raw movies on the device, gains oriented for the movie, sums
written as MRC.

MRC is the container most movies and nearly every gain reference still arrive in; K2 / K3 sessions saved through
SerialEM often hold 4-bit packed samples (mode 101).  This module is the third sibling of ``eer.py`` and ``tiff.py``:

  read_mrc        the 1024-byte MRC2014 header parsed in plain Python -> ``MrcMovie`` (the bytes and where the samples
                  start)
  decode_mrc_raw  the sample rows decoded on the GPU (mc_mrc_decode): the contiguous (t, h, w) movie
  orient_raw      numpy.rot90 + numpy.flip of a raw image or movie on the GPU (mc_raw_orient): the gain reference of
                  one program oriented for the movie of another
  write_mrc       a float image or stack written as an MRC2014 file (host code)
  encode_mrc_raw  a raw uint8 / int16 movie packed into the sample rows of modes 0, 1, 6 and 101 on the GPU
                  (mc_mrc_encode), with the header's statistics from the same pass -> ``MrcMovie``
  write_mrc_raw   that payload written as an MRC2014 file, a chunk of frames at a time

The decoded movie is a raw movie for every ``*_raw*`` function, ``RawStatistics`` and the pipelines, as the outputs
of ``render_eer_raw`` and ``decode_tiff_raw`` are.  The format rule -- the modes and the 4-bit layout -- is stated
once per direction, in csrc/mrc.h and csrc/mrc_encode.h; tests/mrc_reference.py and tests/mrc_encode_reference.py
restate it in numpy.
"""

from __future__ import annotations

import math
import operator
import struct
from dataclasses import dataclass

import torch

from ._files import _check_data, _check_fits_int16, _int, _positive_ints, read_file
from ._lib import check, device_scope, load, ptr, require_gpu, stream_ptr

# mode -> (bytes of a file sample; None for the 4-bit mode, the dtype of the decoded movie)
_MODES = {0: (1, None), 1: (2, torch.int16), 2: (4, torch.float32), 6: (2, torch.int16), 12: (2, torch.float16),
          101: (None, torch.uint8)}
_MODE_NAMES = {3: "complex int16", 4: "complex float32", 7: "int32"}
_IMOD_STAMP = 1146047817
_ORIENT_DTYPES = {torch.uint8: 1, torch.int16: 2, torch.float16: 2, torch.float32: 4}
_FLIPS = {None: 0, "ud": 1, "lr": 2}
_LABEL = b"torch_motion_correction_amd"


def _row_bytes(mode, w):
    return (w + 1) // 2 if mode == 101 else w * _MODES[mode][0]


def _out_dtype(mode, unsigned_bytes):
    if mode == 0:
        return torch.uint8 if unsigned_bytes else torch.int16
    return _MODES[mode][1]


def _check_decode_args(data, offset, shape, mode, swap, unsigned_bytes, flip_rows):
    """Every argument rule of decode_mrc_raw -> (offset, t, h, w, mode) as Python ints; ValueError otherwise."""
    _check_data(data)
    off = _int(offset, "offset", 0)
    t, h, w = _positive_ints(shape, 3, f"shape must be the movie's (t, h, w), three positive ints, got {shape!r}")
    try:
        known = not isinstance(mode, bool) and operator.index(mode) in _MODES
    except TypeError:
        known = False
    if not known:
        raise ValueError(f"mode must be one of 0, 1, 2, 6, 12, 101, got {mode!r}")
    mode = operator.index(mode)
    for name, v in (("swap", swap), ("unsigned_bytes", unsigned_bytes), ("flip_rows", flip_rows)):
        if not isinstance(v, bool):
            raise ValueError(f"{name} must be a bool, got {v!r}")
    if h * w >= 2**31:
        raise ValueError(f"shape {(t, h, w)}: frames of 2^31 samples and more are not supported")
    need = off + t * h * _row_bytes(mode, w)
    if need > data.numel():
        raise ValueError(f"offset {off} + {t} x {h} rows of {_row_bytes(mode, w)} bytes = {need} leaves the "
                         f"{data.numel()} bytes of data")
    return off, t, h, w, mode


def _decode(data, off, t, h, w, mode, swap, unsigned_bytes, flip_rows, device, out=None):
    """The checked arguments decoded -> the (t, h, w) movie on the device.  `out`: a buffer to decode into (the
    tests' guarded buffers)."""
    dev = require_gpu(device if device is not None else data.device)
    dtype = _out_dtype(mode, unsigned_bytes)
    with device_scope(dev):
        buf = data.detach().to(dev).contiguous()
        if out is None:
            out = torch.empty((t, h, w), dtype=dtype, device=dev)
        assert out.dtype == dtype and out.shape == (t, h, w) and out.device == dev
        check(load().mc_mrc_decode(ptr(buf), int(buf.numel()), off, t, h, w, mode, int(swap), int(unsigned_bytes),
                                   int(flip_rows), ptr(out), stream_ptr(dev)), "mc_mrc_decode")
    return out


def decode_mrc_raw(data, offset, shape, mode, swap=False, unsigned_bytes=False, flip_rows=False, device=None):
    """MRC sample rows decoded into a raw movie: the contiguous ``(t, h, w)`` tensor on the GPU.

    ``data``: a 1-D uint8 tensor (CPU or GPU), typically the whole file; the samples start at byte ``offset`` (any
    alignment) and run for ``t * h`` rows without padding.  ``shape``: ``(t, h, w)``.  ``mode``: the MRC mode --

      0    8-bit: ``unsigned_bytes=True`` copies them (uint8), otherwise they are signed and widened to int16
      1    int16
      2    float32 (the gain reference)
      6    uint16, returned as int16 -- the raw routes' 16-bit type; ValueError if a sample is 32768 or more
      12   float16
      101  4-bit, two per byte, a row of ``(w + 1) // 2`` bytes: pixel 2k is the low, pixel 2k + 1 the high nibble of
           byte k (csrc/mrc.h states the rule and what it rests on); uint8, values 0 .. 15

    ``swap``: the file's byte order is not little-endian (modes 1, 2, 6, 12).  ``flip_rows=True`` writes every
    frame's rows in reverse order: MRC's row 0 is the bottom row for the programs that display it, TIFF's the top one.
    The default is stored order, as ``read_tiff`` returns it.

    Exact: the decoder moves bytes.  Every argument rule -- a payload that leaves ``data`` and frames of 2^31 samples
    included -- is a ValueError raised before any device is touched.

    ``device``: the GPU to decode on (None: the device of ``data``, the current GPU for a CPU tensor)."""
    off, t, h, w, mode = _check_decode_args(data, offset, shape, mode, swap, unsigned_bytes, flip_rows)
    movie = _decode(data, off, t, h, w, mode, swap, unsigned_bytes, flip_rows, device)
    if mode == 6:
        _check_fits_int16(movie)
    return movie


@dataclass
class MrcMovie:
    """An MRC file as ``read_mrc`` found it: ``data`` (1-D uint8, the whole file), ``offset`` (the first sample's
    byte: 1024 + nsymbt), ``shape`` (t, h, w) = (nz, ny, nx), ``mode``, ``swap`` (the file is not little-endian),
    ``unsigned_bytes`` (mode 0 holds unsigned bytes, IMOD's convention) and ``pixel_spacing`` (cella.x / mx in
    Angstrom, None when the header does not give it)."""

    data: torch.Tensor
    offset: int
    shape: tuple
    mode: int
    swap: bool
    unsigned_bytes: bool
    pixel_spacing: float | None

    def decode(self, device=None, flip_rows=False):
        """``decode_mrc_raw`` of this movie."""
        return decode_mrc_raw(self.data, self.offset, self.shape, self.mode, swap=self.swap,
                              unsigned_bytes=self.unsigned_bytes, flip_rows=flip_rows, device=device)


def read_mrc(path):
    """An MRC / MRCS file -> ``MrcMovie``: the 1024-byte MRC2014 header parsed in plain Python; no decoder is
    involved.

    The byte order is the machine stamp's (byte 212: 0x44 little, 0x11 big); without a valid stamp it is the order
    under which mapc, mapr, maps are a permutation of 1, 2, 3.  The ``MAP `` word (byte 208) is read and not
    required: files older than MRC2000 lack it.  The extended header (nsymbt bytes) is skipped, not interpreted.
    Mode 0 holds unsigned bytes exactly when imodStamp is 1146047817 and bit 0 of imodFlags is clear (IMOD's
    convention); otherwise they are signed, the MRC2014 rule.

    Refused with a ValueError that names the field and its value: modes 3, 4, 7 and every other mode than 0, 1, 2,
    6, 12, 101; nx, ny or nz below 1; mapc, mapr, maps other than 1, 2, 3; a negative nsymbt; IMOD's older 4-bit
    packing (imodFlags & 16); a file shorter than its header says (bytes beyond the last sample are ignored) or than
    1024 bytes; a bzip2-compressed file.

    Rows are returned in stored order (``MrcMovie.decode(flip_rows=True)`` reverses them)."""
    raw, size, data = read_file(path)

    def fail(msg):
        raise ValueError(f"{path}: {msg}")

    if raw[:3] == b"BZh":
        fail("bzip2-compressed MRC is not decoded")
    if size < 1024:
        fail(f"a file of {size} bytes is shorter than the 1024-byte MRC header")
    orders = {0x44: "<", 0x11: ">"}
    bo = orders.get(raw[212])
    if bo is None:
        for cand in "<>":
            if sorted(struct.unpack_from(cand + "3i", raw, 64)) == [1, 2, 3]:
                bo = cand
                break
        else:
            fail(f"machine stamp 0x{raw[212]:02x} is neither 0x44 nor 0x11, and mapc, mapr, maps = "
                 f"{struct.unpack_from('<3i', raw, 64)} is a permutation of 1, 2, 3 in neither byte order: not an "
                 "MRC file")
    nx, ny, nz, mode = struct.unpack_from(bo + "4i", raw, 0)
    mx = struct.unpack_from(bo + "i", raw, 28)[0]
    cella_x = struct.unpack_from(bo + "f", raw, 40)[0]
    axes = struct.unpack_from(bo + "3i", raw, 64)
    nsymbt = struct.unpack_from(bo + "i", raw, 92)[0]
    imod_stamp, imod_flags = struct.unpack_from(bo + "2i", raw, 152)
    if mode not in _MODES:
        fail(f"mode {mode}" + (f" ({_MODE_NAMES[mode]})" if mode in _MODE_NAMES else "")
             + " is not decoded: 0, 1, 2, 6, 12 and 101 are")
    for name, v in (("nx", nx), ("ny", ny), ("nz", nz)):
        if v < 1:
            fail(f"{name} {v} is below 1")
    if axes != (1, 2, 3):
        fail(f"mapc, mapr, maps = {axes} other than 1, 2, 3: permuted axes are not supported")
    if nsymbt < 0:
        fail(f"nsymbt {nsymbt} is negative")
    imod = imod_stamp == _IMOD_STAMP
    if imod and mode == 0 and imod_flags & 16:
        fail(f"imodFlags {imod_flags}: bit 16, IMOD's older 4-bit packing in mode 0 with nx halved, is not decoded "
             "(mode 101 is)")
    offset = 1024 + nsymbt
    need = offset + nz * ny * _row_bytes(mode, nx)
    if size < need:
        fail(f"a file of {size} bytes is shorter than the {need} its header gives: offset {offset} + nz {nz} x ny "
             f"{ny} rows of {_row_bytes(mode, nx)} bytes")
    spacing = None if mx == 0 or cella_x == 0 else float(cella_x) / mx
    return MrcMovie(data=data, offset=offset, shape=(nz, ny, nx), mode=mode, swap=bo == ">",
                    unsigned_bytes=mode == 0 and imod and not imod_flags & 1, pixel_spacing=spacing)


def _check_orient_args(x, rot90, flip):
    """Every argument rule of orient_raw -> (quarter turns 0..3, flip code); ValueError otherwise."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or x.dtype not in _ORIENT_DTYPES:
        raise ValueError("x must be an (h, w) or (n, h, w) tensor of dtype uint8, int16, float16 or float32, got "
                         f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    if x.numel() == 0:
        raise ValueError(f"x must not be empty, got shape {tuple(x.shape)}")
    k = _int(rot90, "rot90") % 4
    if not (flip is None or isinstance(flip, str)) or flip not in _FLIPS:
        raise ValueError(f"flip must be None, 'ud' or 'lr', got {flip!r}")
    if x.shape[-2] * x.shape[-1] >= 2**31:
        raise ValueError(f"shape {tuple(x.shape)}: images of 2^31 elements and more are not supported")
    return k, _FLIPS[flip]


def _orient(x, k, f, device, out=None):
    dev = require_gpu(device if device is not None else x.device)
    h, w = x.shape[-2:]
    n = x.shape[0] if x.dim() == 3 else 1
    shape = tuple(x.shape[:-2]) + ((w, h) if k & 1 else (h, w))
    with device_scope(dev):
        src = x.detach().to(dev).contiguous()
        if out is None:
            out = torch.empty(shape, dtype=x.dtype, device=dev)
        assert out.dtype == x.dtype and out.shape == shape and out.device == dev
        check(load().mc_raw_orient(ptr(src), _ORIENT_DTYPES[x.dtype], n, h, w, k, f, ptr(out), stream_ptr(dev)),
              "mc_raw_orient")
    return out


def orient_raw(x, rot90=0, flip=None, device=None):
    """A raw image or movie rotated by quarter turns and flipped, on the GPU: the result equals
    ``numpy.rot90(x, rot90, axes=(-2, -1))`` (counter-clockwise) followed by ``numpy.flip`` on axis -2 for
    ``flip="ud"`` or on axis -1 for ``flip="lr"``.

    ``x``: ``(h, w)`` or ``(n, h, w)``, dtype uint8, int16, float16 or float32, on the CPU or a GPU.  ``rot90``: any
    int, taken mod 4.  Returns a new contiguous tensor on the GPU, of shape ``(..., w, h)`` for odd ``rot90``.  Exact:
    elements are moved.  Meant for the gain reference, which must match the movie element for element --
    ``orient_raw(gain, 1, "ud")`` is MotionCor2's ``-RotGain 1 -FlipGain 1`` -- and works equally on a whole raw
    movie, or on a defect map viewed as uint8.

    Every argument rule is a ValueError raised before any device is touched.  ``device``: the GPU to work on (None:
    the device of ``x``, the current GPU for a CPU tensor)."""
    k, f = _check_orient_args(x, rot90, flip)
    return _orient(x, k, f, device)


def write_mrc(path, image, pixel_spacing, dtype=torch.float32):
    """A float image ``(h, w)`` or stack ``(n, h, w)`` (CPU or GPU) written as a little-endian MRC2014 file: mode 2
    for ``dtype=torch.float32``, mode 12 for ``torch.float16``.  Rows are written in the tensor's order.  Returns
    ``path``.

    The header gives nx, ny, nz; mx, my, mz equal to them; cella = (nx, ny, nz) * ``pixel_spacing``; angles of 90;
    mapc, mapr, maps = 1, 2, 3; dmin, dmax, dmean and rms of the values as written, computed in float64; ispg 0;
    nsymbt 0; a blank exttyp; nversion 20140; ``MAP ``; the machine stamp 44 44 00 00; and one label that names this
    package.  ``read_mrc`` reads it back.  Host code: a sum is small next to a movie."""
    if not isinstance(image, torch.Tensor) or not image.is_floating_point() or image.dim() not in (2, 3) \
            or image.numel() == 0:
        raise ValueError("image must be a non-empty float tensor of shape (h, w) or (n, h, w), got "
                         f"{getattr(image, 'dtype', type(image).__name__)} {tuple(getattr(image, 'shape', ()))}")
    if dtype not in (torch.float32, torch.float16):
        raise ValueError(f"dtype must be torch.float32 (mode 2) or torch.float16 (mode 12), got {dtype!r}")
    _check_pixel_spacing(pixel_spacing)
    values = image.detach().to("cpu").to(dtype).contiguous()
    nz = values.shape[0] if values.dim() == 3 else 1
    ny, nx = values.shape[-2:]
    wide = values.double()
    dmean = float(wide.mean())
    rms = math.sqrt(float(((wide - dmean) ** 2).mean()))
    header = _header((nz, ny, nx), 2 if dtype == torch.float32 else 12, pixel_spacing,
                     (float(wide.min()), float(wide.max()), dmean, rms))
    with open(path, "wb") as fh:
        fh.write(header)
        fh.write(values.view(torch.uint8).numpy().tobytes())
    return path


def _check_pixel_spacing(pixel_spacing):
    if isinstance(pixel_spacing, bool) or not isinstance(pixel_spacing, (int, float)) \
            or not math.isfinite(pixel_spacing) or pixel_spacing <= 0:
        raise ValueError(f"pixel_spacing must be a positive number, got {pixel_spacing!r}")


def _header(shape, mode, pixel_spacing, statistics, unsigned_bytes=False):
    """The 1024 header bytes write_mrc describes, for a file of ``shape`` (nz, ny, nx) and ``mode``.  statistics:
    (dmin, dmax, dmean, rms).  unsigned_bytes: IMOD's stamp with imodFlags 0, which marks mode-0 bytes unsigned."""
    nz, ny, nx = shape
    header = bytearray(1024)
    struct.pack_into("<10i", header, 0, nx, ny, nz, mode, 0, 0, 0, nx, ny, nz)
    struct.pack_into("<6f", header, 40, nx * pixel_spacing, ny * pixel_spacing, nz * pixel_spacing, 90.0, 90.0, 90.0)
    struct.pack_into("<3i", header, 64, 1, 2, 3)
    struct.pack_into("<3f", header, 76, *statistics[:3])
    struct.pack_into("<2i", header, 88, 0, 0)  # ispg, nsymbt; exttyp (104) stays blank: four zero bytes
    struct.pack_into("<i", header, 108, 20140)
    if unsigned_bytes:
        struct.pack_into("<2i", header, 152, _IMOD_STAMP, 0)
    header[208:216] = b"MAP \x44\x44\x00\x00"
    struct.pack_into("<f", header, 216, statistics[3])
    struct.pack_into("<i", header, 220, 1)
    header[224:304] = _LABEL.ljust(80)
    return header


# dtype of a raw movie -> (bytes of an element, the mode None stands for, {mode: (lowest, highest) accepted value})
_ENCODE = {torch.uint8: (1, 0, {0: (0, 255), 101: (0, 15)}),
           torch.int16: (2, 1, {1: (-32768, 32767), 6: (0, 32767), 0: (-128, 127), 101: (0, 15)})}
_CHUNK_BYTES = 64 << 20  # of the payload, per device-to-host copy of write_mrc_raw


def _check_encode_args(movie, mode, flip_rows, return_statistics=False):
    """Every argument rule of encode_mrc_raw -> (t, h, w, mode) as Python ints; ValueError otherwise."""
    if not isinstance(movie, torch.Tensor) or movie.dim() not in (2, 3) or movie.dtype not in _ENCODE:
        raise ValueError("movie must be a (t, h, w) or (h, w) tensor of dtype uint8 or int16, got "
                         f"{getattr(movie, 'dtype', type(movie).__name__)} {tuple(getattr(movie, 'shape', ()))}")
    if movie.numel() == 0:
        raise ValueError(f"movie must not be empty, got shape {tuple(movie.shape)}")
    _, default, modes = _ENCODE[movie.dtype]
    if mode is None:
        mode = default
    try:
        known = not isinstance(mode, bool) and operator.index(mode) in modes
    except TypeError:
        known = False
    if not known:
        raise ValueError(f"mode must be None or one of {', '.join(str(m) for m in modes)} for a movie of "
                         f"{movie.dtype}, got {mode!r}")
    for name, v in (("flip_rows", flip_rows), ("return_statistics", return_statistics)):
        if not isinstance(v, bool):
            raise ValueError(f"{name} must be a bool, got {v!r}")
    h, w = movie.shape[-2:]
    if h * w >= 2**31:
        raise ValueError(f"shape {tuple(movie.shape)}: frames of 2^31 samples and more are not supported")
    return (movie.shape[0] if movie.dim() == 3 else 1), h, w, operator.index(mode)


def _scratch_bytes(elem_bytes, t, h, w):
    """csrc/mrc_encode.h's scratch rule: 40 bytes per workgroup, at most 1024 workgroups of 256 per frame"""
    return t * min(1024, -(-h * (w * elem_bytes // 16 + 2) // 256)) * 40


def _encode(movie, t, h, w, mode, flip_rows, device, out=None):
    """The checked arguments encoded -> (the payload on the device, the (t, 5) int64 statistics on the CPU).
    `out`: a uint8 buffer of the payload's size to encode into (the tests' guarded buffers)."""
    dev = require_gpu(device if device is not None else movie.device)
    elem = _ENCODE[movie.dtype][0]
    nbytes = t * h * _row_bytes(mode, w)
    with device_scope(dev):
        src = movie.detach().to(dev).contiguous()
        if out is None:
            out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        assert out.dtype == torch.uint8 and out.shape == (nbytes,) and out.device == dev
        table = torch.empty((t, 5), dtype=torch.int64, device=dev)
        scratch = torch.empty(_scratch_bytes(elem, t, h, w) // 8, dtype=torch.int64, device=dev)
        check(load().mc_mrc_encode(ptr(src), elem, t, h, w, mode, int(flip_rows), ptr(out), nbytes, ptr(table),
                                   ptr(scratch), scratch.numel() * 8, stream_ptr(dev)), "mc_mrc_encode")
        table = table.cpu()
    return out, table


def _refuse_out_of_range(table, dtype, mode):
    """ValueError when the statistics count samples outside the mode's range."""
    bad = sum(table[:, 4].tolist())
    if bad:
        lo, hi = _ENCODE[dtype][2][mode]
        raise ValueError(f"mode {mode} holds values {lo} .. {hi}: {bad} samples of the movie lie outside (its minimum "
                         f"is {min(table[:, 0].tolist())}, its maximum {max(table[:, 1].tolist())})")


def _header_statistics(table, frame_samples):
    """The (t, 5) statistics combined in Python integers -> (dmin, dmax, dmean, rms), rms the root of the mean squared
    deviation from dmean as write_mrc defines it: each the correctly rounded double of an exact rational."""
    rows = table.tolist()
    n = len(rows) * frame_samples
    total, squares = sum(r[2] for r in rows), sum(r[3] for r in rows)
    return (float(min(r[0] for r in rows)), float(max(r[1] for r in rows)), total / n,
            math.sqrt((squares * n - total * total) / (n * n)))


def encode_mrc_raw(movie, mode=None, flip_rows=False, return_statistics=False, device=None):
    """A raw movie encoded as MRC sample rows -> ``MrcMovie``: the inverse of ``decode_mrc_raw`` for the integer
    types, and what ``write_mrc_raw`` puts into a file.

    ``movie``: ``(t, h, w)``, or ``(h, w)`` for one image; ``torch.uint8`` or ``int16``, CPU or GPU, any strides (it
    is made contiguous).  ``mode`` (None: 0 for uint8, 1 for int16):

      uint8   0    the bytes, marked unsigned (``unsigned_bytes=True``: IMOD's convention, as ``read_mrc`` takes it)
      uint8   101  4-bit; values 0 .. 15
      int16   1    int16
      int16   6    uint16; values 0 .. 32767
      int16   0    signed bytes, the MRC2014 rule; values -128 .. 127
      int16   101  4-bit; values 0 .. 15

    Mode 101 packs two pixels per byte, a row of ``(w + 1) // 2`` bytes, pixel 2k the low and pixel 2k + 1 the high
    nibble of byte k, the last high nibble of a row of odd ``w`` 0 (csrc/mrc_encode.h states the rule and what it rests
    on).  ``flip_rows=True`` writes every frame's rows in reverse order, the inverse of the decoder's option.

    One pass on the GPU (mc_mrc_encode) packs the samples and gathers, exactly in 64-bit integers, each frame's
    minimum, maximum, sum, sum of squares and the count of samples outside the mode's range.  A movie with such
    samples is a ValueError that names the mode, the count and the movie's minimum and maximum; nothing is wrapped
    silently.  The returned movie has ``data`` = the payload, 1-D uint8 on the GPU, ``offset`` 0, ``shape``
    ``(t, h, w)``, ``mode``, ``swap=False``, ``unsigned_bytes`` True exactly for uint8 -> mode 0 and
    ``pixel_spacing=None``; ``.decode()`` gives the movie back: int16 for modes 1, 6 and the signed mode 0, uint8 for
    the unsigned mode 0 and mode 101.  ``return_statistics=True``: ``(movie, table)`` with the ``(t, 5)`` int64 table
    of the five statistics on the CPU.  There is one device-to-host read, of that table.

    Every argument rule is a ValueError raised before any device is touched.  ``device``: the GPU to encode on (None:
    the device of ``movie``, the current GPU for a CPU tensor)."""
    t, h, w, mode = _check_encode_args(movie, mode, flip_rows, return_statistics)
    payload, table = _encode(movie, t, h, w, mode, flip_rows, device)
    _refuse_out_of_range(table, movie.dtype, mode)
    out = MrcMovie(data=payload, offset=0, shape=(t, h, w), mode=mode, swap=False,
                   unsigned_bytes=movie.dtype == torch.uint8 and mode == 0, pixel_spacing=None)
    return (out, table) if return_statistics else out


def write_mrc_raw(path, movie, pixel_spacing, mode=None, flip_rows=False, device=None):
    """A raw movie (uint8 or int16, ``(t, h, w)`` or ``(h, w)``, CPU or GPU) written as a little-endian MRC2014 file
    of ``mode`` 0, 1, 6 or 101: ``encode_mrc_raw(movie, mode, flip_rows, device=device)`` on the GPU, then host code
    for the header and the file.  Returns ``path``.

    The header is ``write_mrc``'s, with the mode, with dmin, dmax, dmean and rms from the pass's exact integer
    statistics combined in Python integers (rms: the root of the mean squared deviation), and, for uint8 -> mode 0,
    imodStamp 1146047817 with imodFlags 0, so that ``read_mrc`` and IMOD take the bytes as unsigned.  The payload
    comes to the host in chunks of whole frames of about 64 MiB; there is no second copy of the movie on the host.
    A movie that is refused -- an argument rule, or samples outside the mode's range -- leaves nothing at ``path``.
    ``read_mrc`` reads what this writes."""
    _check_pixel_spacing(pixel_spacing)
    encoded, table = encode_mrc_raw(movie, mode=mode, flip_rows=flip_rows, return_statistics=True, device=device)
    t, h, w = encoded.shape
    header = _header(encoded.shape, encoded.mode, pixel_spacing, _header_statistics(table, h * w),
                     encoded.unsigned_bytes)
    frame_bytes = encoded.data.numel() // t
    frames = max(1, _CHUNK_BYTES // frame_bytes)
    with open(path, "wb") as fh:
        fh.write(header)
        for f in range(0, t, frames):
            fh.write(memoryview(encoded.data[f * frame_bytes:(f + frames) * frame_bytes].cpu().numpy()))
    return path
