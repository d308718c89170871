"""TIFF 6.0 LZW restated with Python integers: the sequential decoder the device decode (mc_tiff_decode) is compared
with, an encoder that produces test streams, and the strip-movie flavour of the container writer
(tests/tiff_files.py).  The rule is the one csrc/tiff_lzw.h states; tests/golden/tiff_lzw_libtiff.npz pins it to files
libtiff wrote.

  codes packed MSB-first; width 9 at the start and after Clear (256); EOI = 257; first free code 258
  the decoder starts cleared whether or not the stream begins with Clear
  a code with a previous code present adds entry `next` = previous string + first byte of this string
  early change: after the add, next + 1 >= 1 << width and width < 12 -> width += 1
  c == next is KwKwK; c > next, or c >= 256 with no previous code, is malformed: stop
  entries are added only while next < 4096; beyond that decoding goes on at 12 bits
  stop at EOI, at the expected size, when fewer than `width` bits are left, at a malformed code
"""

import tiff_files

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


lay_out = tiff_files.lay_out


def write_tiff(path, strips, shape, rows_per_strip, big=False, byte_order="<", compression=5, bits=8,
               sample_format=1, array_type=4, overrides=None, loop=False):
    """tiff_files.write_tiff with a strip movie's tags; StripOffsets and StripByteCounts have TIFF type `array_type`.
    Returns (offsets, nbytes) per frame."""
    tags = {256: (4, 1, shape[1]), 257: (4, 1, shape[0]), 258: (3, 1, bits), 259: (3, 1, compression),
            278: (4, 1, rows_per_strip), 339: (3, 1, sample_format)}
    return tiff_files.write_tiff(path, strips, tags, big=big, byte_order=byte_order,
                                 array_types=(array_type, array_type), overrides=overrides, loop=loop)
