"""An independent restatement of the MRC rule of csrc/mrc.h and torch_motion_correction_amd/mrc.py in numpy and
struct: a writer of MRC2014 files for every mode the package decodes (and any other mode number), in either byte
order, with or without IMOD's stamp and flags, with an extended header of any length and with any header field
overridden; the decoder as numpy expressions; the orientation as numpy.rot90 / numpy.flip.  Nothing here imports the
package.

The 4-bit layout (mode 101) is the one the IMOD / MRC2014 format descriptions give: a row is (nx + 1) // 2 bytes,
pixel 2k the low nibble of byte k, pixel 2k + 1 the high nibble.  It is a reading of those descriptions, not of a
file written by IMOD or SerialEM."""

import struct

import numpy as np

IMOD_STAMP = 1146047817
LABEL = b"torch_motion_correction_amd"
# mode -> the dtype of the file's samples (None: 4-bit)
FILE_DTYPES = {0: np.dtype("u1"), 1: np.dtype("i2"), 2: np.dtype("f4"), 6: np.dtype("u2"), 12: np.dtype("f2"),
               101: None}
# header fields by name -> (byte offset, struct code)
FIELDS = {"nx": (0, "i"), "ny": (4, "i"), "nz": (8, "i"), "mode": (12, "i"), "mx": (28, "i"), "my": (32, "i"),
          "mz": (36, "i"), "cella_x": (40, "f"), "mapc": (64, "i"), "mapr": (68, "i"), "maps": (72, "i"),
          "nsymbt": (92, "i"), "imodStamp": (152, "i"), "imodFlags": (156, "i")}


def row_bytes(mode, nx):
    return (nx + 1) // 2 if mode == 101 else nx * FILE_DTYPES[mode].itemsize


def pack_rows(pixels, mode, byte_order="<", pad_nibble=0):
    """(t, h, w) pixel values -> the file's sample bytes.  mode 0 takes int8 or uint8 values as they are; mode 101
    takes values 0 .. 15 and fills the padding nibble of odd rows with `pad_nibble`."""
    pixels = np.asarray(pixels)
    if mode == 101:
        t, h, w = pixels.shape
        assert pixels.min() >= 0 and pixels.max() <= 15
        padded = np.full((t, h, 2 * ((w + 1) // 2)), pad_nibble, dtype=np.uint8)
        padded[:, :, :w] = pixels
        return (padded[:, :, 0::2] | (padded[:, :, 1::2] << 4)).astype(np.uint8).tobytes()
    if mode == 0:
        assert pixels.dtype.itemsize == 1
        return pixels.tobytes()
    return pixels.astype(FILE_DTYPES[mode].newbyteorder(byte_order)).tobytes()


def header(shape, mode, byte_order="<", stamp=True, imod=None, nsymbt=0, pixel_spacing=None, overrides=None,
           stats=(0.0, 0.0, 0.0, 0.0), label=None):
    """The 1024 header bytes.  shape: (nz, ny, nx).  stamp: write the machine stamp (False: four zero bytes).
    imod: None, or the imodFlags to write beside IMOD's stamp.  overrides: {field name of FIELDS: value}, written
    last."""
    nz, ny, nx = shape
    bo = byte_order
    h = bytearray(1024)
    struct.pack_into(bo + "10i", h, 0, nx, ny, nz, mode, 0, 0, 0, nx, ny, nz)
    sp = 0.0 if pixel_spacing is None else pixel_spacing
    struct.pack_into(bo + "6f", h, 40, nx * sp, ny * sp, nz * sp, 90.0, 90.0, 90.0)
    struct.pack_into(bo + "3i", h, 64, 1, 2, 3)
    struct.pack_into(bo + "3f", h, 76, *stats[:3])
    struct.pack_into(bo + "2i", h, 88, 0, nsymbt)
    struct.pack_into(bo + "i", h, 108, 20140)
    if imod is not None:
        struct.pack_into(bo + "2i", h, 152, IMOD_STAMP, imod)
    h[208:212] = b"MAP "
    if stamp:
        h[212:216] = b"\x44\x44\x00\x00" if bo == "<" else b"\x11\x11\x00\x00"
    struct.pack_into(bo + "f", h, 216, stats[3])
    if label is not None:
        struct.pack_into(bo + "i", h, 220, 1)
        h[224:304] = label.ljust(80)
    for name, value in (overrides or {}).items():
        at, code = FIELDS[name]
        struct.pack_into(bo + code, h, at, value)
    return bytes(h)


def write_mrc(path, pixels, mode, byte_order="<", stamp=True, imod=None, nsymbt=0, pixel_spacing=None,
              overrides=None, ext_fill=0xEE, trailing=b"", pad_nibble=0, payload=None):
    """An MRC file of (t, h, w) `pixels` -> the file's bytes (also written to `path` unless it is None).  The
    extended header is `nsymbt` bytes of `ext_fill`; `payload` replaces the sample bytes (a mode the package
    refuses)."""
    pixels = np.asarray(pixels)
    body = pack_rows(pixels, mode, byte_order, pad_nibble) if payload is None else payload
    raw = header(pixels.shape, mode, byte_order, stamp, imod, nsymbt, pixel_spacing, overrides) \
        + bytes([ext_fill]) * max(nsymbt, 0) + body + trailing
    if path is not None:
        with open(path, "wb") as fh:
            fh.write(raw)
    return raw


def decode(payload, shape, mode, swap=False, unsigned_bytes=False, flip_rows=False):
    """The rule: the sample bytes of a (t, h, w) movie -> the array decode_mrc_raw returns (mode 6 as int16 by
    reinterpretation; the caller refuses samples >= 32768)."""
    t, h, w = shape
    rb = row_bytes(mode, w)
    rows = np.frombuffer(payload, dtype=np.uint8, count=t * h * rb).reshape(t, h, rb)
    if mode == 101:
        out = np.empty((t, h, 2 * rb), dtype=np.uint8)
        out[:, :, 0::2] = rows & 15
        out[:, :, 1::2] = rows >> 4
        out = out[:, :, :w]
    elif mode == 0:
        out = rows.copy() if unsigned_bytes else rows.view(np.int8).astype(np.int16)
    else:
        dt = {1: "i2", 2: "f4", 6: "i2", 12: "f2"}[mode]
        out = np.ascontiguousarray(rows).view(np.dtype(dt).newbyteorder(">" if swap else "<")).astype(np.dtype(dt))
    if flip_rows:
        out = out[:, ::-1, :]
    return np.array(out, order="C")  # a copy: a view of one row keeps its negative stride through ascontiguousarray


def orient(x, rot90=0, flip=None):
    out = np.rot90(x, rot90, axes=(-2, -1))
    if flip is not None:
        out = np.flip(out, axis={"ud": -2, "lr": -1}[flip])
    return np.array(out, order="C")


def written_by_write_mrc(image, pixel_spacing, dtype):
    """The bytes write_mrc must produce for `image` ((h, w) or (n, h, w) float array) as numpy `dtype` (f4 / f2)."""
    values = np.asarray(image).astype(dtype)
    stack = values if values.ndim == 3 else values[None]
    wide = stack.astype(np.float64)
    mean = float(wide.mean())
    stats = (float(wide.min()), float(wide.max()), mean, float(np.sqrt(((wide - mean) ** 2).mean())))
    mode = 2 if np.dtype(dtype) == np.dtype("f4") else 12
    return header(stack.shape, mode, pixel_spacing=pixel_spacing, stats=stats, label=LABEL) \
        + stack.astype(np.dtype(dtype).newbyteorder("<")).tobytes()
