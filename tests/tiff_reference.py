"""TIFF 6.0 LZW restated with Python integers: the sequential decoder the device decode (mc_tiff_decode) is compared
with, an encoder that produces test streams, and a writer of minimal multi-strip TIFF / BigTIFF files.  The rule is
the one csrc/tiff_lzw.h states; tests/golden/tiff_lzw_libtiff.npz pins it to files libtiff wrote.

  codes packed MSB-first; width 9 at the start and after Clear (256); EOI = 257; first free code 258
  the decoder starts cleared whether or not the stream begins with Clear
  a code with a previous code present adds entry `next` = previous string + first byte of this string
  early change: after the add, next + 1 >= 1 << width and width < 12 -> width += 1
  c == next is KwKwK; c > next, or c >= 256 with no previous code, is malformed: stop
  entries are added only while next < 4096; beyond that decoding goes on at 12 bits
  stop at EOI, at the expected size, when fewer than `width` bits are left, at a malformed code
"""

import struct

CLEAR, EOI, FIRST, TABLE = 256, 257, 258, 4096
STOPS = ("eoi", "full", "bits", "malformed")


def decode_strip(data, expected, trace=None):
    """The strip's bytes decoded -> (at most `expected` bytes, why decoding stopped: one of STOPS).  `trace`: a list
    that gets (code, width it was read with, next before it) per code."""
    data = bytes(data)
    nbits = 8 * len(data)
    value = int.from_bytes(data, "big")
    out = bytearray()
    table = {}
    width, nxt, prev, bit = 9, FIRST, None, 0
    while True:
        if len(out) >= expected:
            return bytes(out[:expected]), "full"
        if nbits - bit < width:
            return bytes(out), "bits"
        c = (value >> (nbits - bit - width)) & ((1 << width) - 1)
        if trace is not None:
            trace.append((c, width, nxt))
        bit += width
        if c == CLEAR:
            table, width, nxt, prev = {}, 9, FIRST, None
            continue
        if c == EOI:
            return bytes(out), "eoi"
        if c < 256:
            s = bytes([c])
        elif prev is None or c > nxt:
            return bytes(out), "malformed"
        elif c == nxt:
            s = prev + prev[:1]
        else:
            s = table[c]
        if prev is not None and nxt < TABLE:
            table[nxt] = prev + s[:1]
            nxt += 1
            if nxt + 1 >= (1 << width) and width < 12:
                width += 1
        out += s
        prev = s


class _Bits:
    def __init__(self):
        self.value, self.n = 0, 0

    def put(self, v, k):
        self.value = (self.value << k) | v
        self.n += k

    def bytes(self):
        pad = -self.n % 8
        return (self.value << pad).to_bytes((self.n + pad) // 8, "big")


def encode_strip(data, leading_clear=True, eoi=True, defer_clear=0, clear_at=None):
    """`data` as one LZW strip.  The table is cleared the way libtiff clears it, when entry 4093 has been added,
    unless `defer_clear` = n > 0: then the table fills up, n more codes follow at 12 bits with nothing added, and
    only then Clear.  `clear_at`: a Clear is also forced after that many codes (counted since the last Clear)."""
    data = bytes(data)
    bits = _Bits()
    # the decoder's state, kept in step: width for the next code, its next free code, whether it has a previous code
    state = {}

    def reset():
        state.update(width=9, nxt=FIRST, prev=False, codes=0, full=0)
        table.clear()

    def emit(c):
        bits.put(c, state["width"])
        if c == CLEAR:
            reset()
            return
        if state["prev"] and state["nxt"] < TABLE:
            state["nxt"] += 1
            if state["nxt"] + 1 >= (1 << state["width"]) and state["width"] < 12:
                state["width"] += 1
        state["prev"] = True
        state["codes"] += 1

    table = {}
    reset()
    if leading_clear:
        emit(CLEAR)
    i, n = 0, len(data)
    while i < n:
        # the longest string in the table that begins at i
        c, j = data[i], i + 1
        while j < n and (c, data[j]) in table:
            c, j = table[c, data[j]], j + 1
        emit(c)
        # the entry the decoder adds when it reads the NEXT code: its number is the decoder's `next` now
        if j < n and state["nxt"] < TABLE:
            table[c, data[j]] = state["nxt"]
        i = j
        if i >= n:
            break
        if state["nxt"] >= TABLE:
            state["full"] += 1
        if defer_clear:
            if state["full"] > defer_clear:
                emit(CLEAR)
        elif state["nxt"] >= 4093:
            emit(CLEAR)
        if clear_at is not None and state["codes"] >= clear_at:
            emit(CLEAR)
    if eoi:
        bits.put(EOI, state["width"])
    return bits.bytes()


def strips_of(frame_bytes, row_bytes, rows_per_strip):
    """one frame's bytes cut into the byte strings of its strips"""
    step = row_bytes * rows_per_strip
    return [frame_bytes[k:k + step] for k in range(0, len(frame_bytes), step)]


def encode_movie(movie, rows_per_strip, **kw):
    """A (t, h, w) numpy movie -> per frame the list of its LZW strips."""
    t, h, w = movie.shape
    row_bytes = w * movie.dtype.itemsize
    return [[encode_strip(s, **kw) for s in strips_of(frame.tobytes(), row_bytes, rows_per_strip)]
            for frame in movie]


def decode_movie(strips, shape, rows_per_strip, row_bytes):
    """The sequential reference of decode_tiff_raw -> (bytes of the movie with zeros where a strip gave nothing,
    per-strip bytes produced)."""
    h = shape[0]
    out, produced = bytearray(), []
    for frame in strips:
        for k, s in enumerate(frame):
            want = min(rows_per_strip, h - k * rows_per_strip) * row_bytes
            got, _ = decode_strip(s, want)
            produced.append(len(got))
            out += got + bytes(want - len(got))
    return bytes(out), produced


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


# ------------------------------------------------------------------ containers

_SIZES = {1: 1, 3: 2, 4: 4, 16: 8}
_CODES = {1: "B", 3: "H", 4: "I", 16: "Q"}


def write_tiff(path, strips, shape, rows_per_strip, big=False, byte_order="<", compression=5, bits=8,
               sample_format=1, array_type=4, overrides=None, loop=False):
    """A minimal TIFF (magic 42) or BigTIFF (magic 43): one IFD per frame, `strips[f]` its strips, written in
    reverse order at odd offsets, each frame's IFD and its out-of-line arrays behind its strips.  StripOffsets and
    StripByteCounts have TIFF type `array_type` (3 SHORT, 4 LONG, 16 LONG8) and go inline when they fit the value
    field.  `overrides[frame][tag]` = (type, count, value or list) replaces or adds an entry, None drops it.  `loop`:
    the last IFD points back at the first.  Returns (offsets, nbytes) per frame."""
    h, w = shape
    bo, n = byte_order, len(strips)
    overrides = overrides or {}
    fsz = 8 if big else 4
    out = bytearray(16 if big else 8)
    strip_at = [[0] * len(f) for f in strips]
    ifd_at = [0] * n
    blobs = []
    for i in reversed(range(n)):
        for k in reversed(range(len(strips[i]))):
            if len(out) % 2 == 0:
                out += b"\xee"
            strip_at[i][k] = len(out)
            out += strips[i][k]
        e = {256: (4, 1, w), 257: (4, 1, h), 258: (3, 1, bits), 259: (3, 1, compression),
             273: (array_type, len(strips[i]), strip_at[i]), 278: (4, 1, rows_per_strip),
             279: (array_type, len(strips[i]), [len(s) for s in strips[i]]), 339: (3, 1, sample_format)}
        for tag, val in overrides.get(i, {}).items():
            if val is None:
                e.pop(tag, None)
            else:
                e[tag] = val
        fields = []
        for tag, (typ, count, value) in sorted(e.items()):
            vals = list(value) if isinstance(value, (list, tuple)) else [value]
            field = bytearray(fsz)
            if typ in _SIZES and _SIZES[typ] * count <= fsz and len(vals) == count:
                struct.pack_into(f"{bo}{count}{_CODES[typ]}", field, 0, *vals)
            elif typ in _SIZES and len(vals) == count:  # out of line
                out += b"\xee" * (len(out) % 2)
                struct.pack_into(bo + ("Q" if big else "I"), field, 0, len(out))
                out += struct.pack(f"{bo}{count}{_CODES[typ]}", *vals)
            else:  # a raw value field: an offset the test chose, or a type the reader refuses
                struct.pack_into(bo + ("Q" if big else "I"), field, 0, vals[0])
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
            struct.pack_into(bo + "HH" + ("Q" if big else "I"), out, p, tag, typ, count)
            out[p + 4 + fsz:p + 4 + 2 * fsz] = field
            p += 4 + 2 * fsz
        nxt = ifd_at[i + 1] if i + 1 < n else (ifd_at[0] if loop else 0)
        struct.pack_into(bo + ("Q" if big else "I"), out, p, nxt)
    out[:2] = b"II" if bo == "<" else b"MM"
    if big:
        struct.pack_into(bo + "HHHQ", out, 2, 43, 8, 0, ifd_at[0] if n else 0)
    else:
        struct.pack_into(bo + "HI", out, 2, 42, ifd_at[0] if n else 0)
    with open(path, "wb") as fh:
        fh.write(out)
    return strip_at, [[len(s) for s in f] for f in strips]
