"""What the movie-file modules (eer.py, tiff.py, mrc.py) share, stated once: the file read into one writable buffer,
the argument rules every decoder starts with, and the walk of a TIFF / BigTIFF IFD chain.  Host code only: nothing here
touches a device -- staging stays in each format module, next to its entry point.
"""

from __future__ import annotations

import operator
import os
import struct

import torch

_INT_TYPES = {1: "B", 3: "H", 4: "I", 16: "Q"}  # TIFF types BYTE, SHORT, LONG, LONG8
STRIP_TAGS = (256, 257, 259, 273, 279)          # what every IFD of strips must give


def read_file(path):
    """-> (raw, size, data): the file's bytes as a bytearray, their number, and the 1-D uint8 tensor that SHARES the
    bytearray -- a movie file is 0.5 - 1 GB, and there is one copy of it."""
    with open(path, "rb") as fh:
        raw = bytearray(os.fstat(fh.fileno()).st_size)  # writable, so that the tensor below shares it
        size = fh.readinto(raw)
    if size != len(raw):
        del raw[size:]
    data = torch.frombuffer(raw, dtype=torch.uint8) if size else torch.empty(0, dtype=torch.uint8)
    return raw, size, data


def _int(value, what, lo=None):
    """`value` as a Python int (bools refused), at least `lo` where one is given; ValueError otherwise."""
    if not isinstance(value, bool):
        try:
            v = operator.index(value)
        except TypeError:
            v = None
        if v is not None and (lo is None or v >= lo):
            return v
    raise ValueError(f"{what} must be an int" + ("" if lo is None else f" >= {lo}") + f", got {value!r}")


def _positive_ints(shape, n, message):
    """`shape` as `n` positive Python ints (bools refused); ValueError(`message`) otherwise."""
    try:
        dims = [_int(s, "a size", 1) for s in shape]
    except (TypeError, ValueError):
        dims = []
    if len(dims) != n:
        raise ValueError(message)
    return dims


def _check_data(data):
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8 or data.dim() != 1:
        raise ValueError("data must be a 1-D uint8 tensor, got "
                         f"{getattr(data, 'dtype', type(data).__name__)} {tuple(getattr(data, 'shape', ()))}")


def _check_fits_int16(movie):
    """`movie`: unsigned 16-bit samples decoded as int16."""
    if bool((movie < 0).any()):
        raise ValueError("an unsigned 16-bit sample is 32768 or more: the movie does not fit the raw routes' int16")


def walk_ifds(raw, size, names, fail):
    """The IFD chain of a TIFF (magic 42) or BigTIFF (magic 43) file in either byte order: a generator of one dict per
    IFD, ``{tag: (TIFF type, [values])}`` for the tags in `names` (tag -> its name in messages); other tags are not
    looked at.  Values are unsigned integers (BYTE, SHORT, LONG, LONG8), inline or out of line.  ``fail(message)``
    must raise: it is called for a file that is no TIFF, a chain that loops, an IFD or out-of-line values outside
    the `size` bytes of `raw`, a value of another type or without values, and a file without any IFD."""
    if size < 8 or raw[:2] not in (b"II", b"MM"):
        fail("not a TIFF file (byte order mark)")
    bo = "<" if raw[:2] == b"II" else ">"
    magic = struct.unpack_from(bo + "H", raw, 2)[0]
    if magic == 42:
        entry_size, count_fmt, off_fmt = 12, "H", "I"
        ifd = struct.unpack_from(bo + "I", raw, 4)[0]
    elif magic == 43:
        if size < 16 or struct.unpack_from(bo + "HH", raw, 4) != (8, 0):
            fail("BigTIFF header with an offset size other than 8")
        entry_size, count_fmt, off_fmt = 20, "Q", "Q"
        ifd = struct.unpack_from(bo + "Q", raw, 8)[0]
    else:
        fail(f"TIFF magic {magic} is neither 42 (TIFF) nor 43 (BigTIFF)")
    csz, osz = struct.calcsize(count_fmt), struct.calcsize(off_fmt)
    seen = set()
    while ifd:
        i = len(seen)
        if ifd in seen:
            fail(f"frame {i}: the IFD chain loops")
        seen.add(ifd)
        if ifd + csz > size:
            fail(f"frame {i}: its IFD lies outside the file")
        n_entries = struct.unpack_from(bo + count_fmt, raw, ifd)[0]
        end = ifd + csz + n_entries * entry_size
        if end + osz > size:
            fail(f"frame {i}: its IFD lies outside the file")
        tags = {}
        for at in range(ifd + csz, end, entry_size):
            tag, typ = struct.unpack_from(bo + "HH", raw, at)
            if tag not in names:
                continue
            where = f"frame {i}: {names[tag]}"
            count = struct.unpack_from(bo + off_fmt, raw, at + 4)[0]
            if typ not in _INT_TYPES:
                fail(f"{where} has TIFF type {typ}, not one of {sorted(_INT_TYPES)} (unsigned integers)")
            if count < 1:
                fail(f"{where} has no value")
            at += 4 + osz
            width = struct.calcsize(_INT_TYPES[typ])
            if width * count > osz:  # out of line
                at = struct.unpack_from(bo + off_fmt, raw, at)[0]
                if at + width * count > size:
                    fail(f"{where}: its {count} values at offset {at} leave the file of {size} bytes")
            tags[tag] = (typ, list(struct.unpack_from(f"{bo}{count}{_INT_TYPES[typ]}", raw, at)))
        yield tags
        ifd = struct.unpack_from(bo + off_fmt, raw, end)[0]
    if not seen:
        fail("the file holds no frame (no IFD)")


def require_tags(tags, names, i, fail, required=STRIP_TAGS):
    for tag in required:
        if tag not in tags:
            fail(f"frame {i}: {names[tag]} is missing")
