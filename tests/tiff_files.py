"""TIFF / BigTIFF files for the tests of eer.py and tiff.py, stated once: a writer of minimal multi-strip files with
every liberty the readers must cope with, a layout of strips in one buffer, and a struct walk of a file's IFDs that
shares nothing with the package's own walker.  tests/eer_reference.py and tests/tiff_reference.py give the writer
their formats' tags."""

import struct

_CODES = {1: "B", 3: "H", 4: "I", 16: "Q"}  # TIFF types BYTE, SHORT, LONG, LONG8


def lay_out(strips, order=None, lead=1, gap=3, odd=True, fill=None):
    """Every strip of every frame laid into one buffer in `order` (indices into the flattened frame-major list),
    `gap` bytes between them (0xff, or bytes drawn from the numpy generator `fill`), every strip at an odd offset
    when `odd` -> (bytes, offsets, nbytes), the latter two as lists per frame."""
    flat = [s for f in strips for s in f]
    order = range(len(flat)) if order is None else order

    def pad(k):
        return bytes(fill.integers(0, 256, k, dtype="uint8")) if fill is not None else b"\xff" * k

    buf = bytearray(pad(lead))
    at = [0] * len(flat)
    for i in order:
        buf += pad(gap)
        if odd and len(buf) % 2 == 0:
            buf += pad(1)
        at[i] = len(buf)
        buf += flat[i]
    buf += pad(gap)
    offsets, nbytes, i = [], [], 0
    for f in strips:
        offsets.append(at[i:i + len(f)])
        nbytes.append([len(s) for s in f])
        i += len(f)
    return bytes(buf), offsets, nbytes


def write_tiff(path, strips, tags, big=False, byte_order="<", order=None, array_types=(4, 4), overrides=None,
               loop=False):
    """A minimal TIFF (magic 42) or BigTIFF (magic 43): one IFD per frame, `strips[f]` its strips.  The frames are
    written in `order` (default: reversed), a frame's strips in reverse, every strip at an odd offset, each frame's
    out-of-line arrays and its IFD behind its strips at even offsets: IFD bytes lie between strips and the IFD chain
    jumps back and forth.  `tags`: the entries every IFD has besides StripOffsets and StripByteCounts, which get the
    TIFF types `array_types` (3 SHORT, 4 LONG, 16 LONG8); values go inline when they fit the value field.
    `overrides[frame][tag]` = (type, count, value or list) replaces or adds an entry, None drops it; a value that is
    not `count` integers of a known type is written into the value field as it is -- an offset the test chose, or a
    type the reader refuses.  `loop`: the last IFD points back at the first.  Returns (offsets, nbytes) per frame."""
    bo, n = byte_order, len(strips)
    order = list(reversed(range(n))) if order is None else list(order)
    overrides = overrides or {}
    word, fsz = ("Q", 8) if big else ("I", 4)
    out = bytearray(16 if big else 8)
    strip_at = [[0] * len(f) for f in strips]
    ifd_at = [0] * n
    blobs = []
    for i in order:
        for k in reversed(range(len(strips[i]))):
            if len(out) % 2 == 0:
                out += b"\xee"
            strip_at[i][k] = len(out)
            out += strips[i][k]
        e = {**tags, 273: (array_types[0], len(strips[i]), strip_at[i]),
             279: (array_types[1], len(strips[i]), [len(s) for s in strips[i]])}
        for tag, val in overrides.get(i, {}).items():
            if val is None:
                e.pop(tag, None)
            else:
                e[tag] = val
        fields = []
        for tag, (typ, count, value) in sorted(e.items()):
            vals = list(value) if isinstance(value, (list, tuple)) else [value]
            field = bytearray(fsz)
            size = struct.calcsize(_CODES[typ]) * count if typ in _CODES and len(vals) == count else None
            if size is None:  # a raw value field
                struct.pack_into(bo + word, field, 0, vals[0])
            elif size <= fsz:
                struct.pack_into(f"{bo}{count}{_CODES[typ]}", field, 0, *vals)
            else:  # out of line
                out += b"\xee" * (len(out) % 2)
                struct.pack_into(bo + word, field, 0, len(out))
                out += struct.pack(f"{bo}{count}{_CODES[typ]}", *vals)
            fields.append((tag, typ, count, field))
        out += b"\xee" * (len(out) % 2)
        ifd_at[i] = len(out)
        out += bytes((8 if big else 2) + (4 + 2 * fsz) * len(fields) + fsz)
        blobs.append((i, fields))
    for i, fields in blobs:
        p = ifd_at[i]
        struct.pack_into(bo + ("Q" if big else "H"), out, p, len(fields))
        p += 8 if big else 2
        for tag, typ, count, field in fields:
            struct.pack_into(bo + "HH" + word, out, p, tag, typ, count)
            out[p + 4 + fsz:p + 4 + 2 * fsz] = field
            p += 4 + 2 * fsz
        struct.pack_into(bo + word, out, p, ifd_at[i + 1] if i + 1 < n else (ifd_at[0] if loop else 0))
    out[:2] = b"II" if bo == "<" else b"MM"
    if big:
        struct.pack_into(bo + "HHHQ", out, 2, 43, 8, 0, ifd_at[0] if n else 0)
    else:
        struct.pack_into(bo + "HI", out, 2, 42, ifd_at[0] if n else 0)
    with open(path, "wb") as fh:
        fh.write(out)
    return strip_at, [[len(s) for s in f] for f in strips]


def walk_ifds(raw):
    """A struct walk of a well-formed TIFF / BigTIFF in either byte order, independent of the package's readers ->
    (big, [(IFD offset, [(tag, type, count, values)])]); values is None for a type that holds no unsigned
    integers.  Out-of-line values must begin on a word boundary, as TIFF 6.0 requires."""
    bo = {b"II": "<", b"MM": ">"}[bytes(raw[:2])]
    magic = struct.unpack_from(bo + "H", raw, 2)[0]
    big = magic == 43
    if big:
        assert struct.unpack_from(bo + "HH", raw, 4) == (8, 0)
    else:
        assert magic == 42
    word, wsz, cnt, entry = ("Q", 8, 8, 20) if big else ("I", 4, 2, 12)
    ifd = struct.unpack_from(bo + word, raw, wsz)[0]
    out = []
    while ifd:
        n = struct.unpack_from(bo + ("Q" if big else "H"), raw, ifd)[0]
        tags = []
        for k in range(n):
            at = ifd + cnt + entry * k
            tag, typ, count = struct.unpack_from(bo + "HH" + word, raw, at)
            values = None
            if typ in _CODES:
                field = at + 4 + wsz
                if struct.calcsize(_CODES[typ]) * count > wsz:
                    field = struct.unpack_from(bo + word, raw, field)[0]
                    assert field % 2 == 0
                values = list(struct.unpack_from(f"{bo}{count}{_CODES[typ]}", raw, field))
            tags.append((tag, typ, count, values))
        out.append((ifd, tags))
        ifd = struct.unpack_from(bo + word, raw, ifd + cnt + entry * n)[0]
    return big, out
