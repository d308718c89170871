"""An independent restatement of the MRC encode rule of csrc/mrc_encode.h in numpy: the payload bytes of a raw movie
for every (dtype, mode) pair of the table below, the five statistics per frame, and the header's four statistics in
float64.  Nothing here imports the package.

  movie   mode   file sample                       accepted values
  uint8   0      the byte (unsigned, IMOD's way)   all
  uint8   101    4-bit                             0 .. 15
  int16   1      the two bytes, little-endian      all
  int16   6      the same two bytes                0 .. 32767
  int16   0      one signed byte                   -128 .. 127
  int16   101    4-bit                             0 .. 15

Mode 101: a row is (w + 1) // 2 bytes, pixel 2k the low nibble of byte k, pixel 2k + 1 the high nibble, the last high
nibble of a row of odd w 0 -- the reading of the IMOD / MRC2014 format descriptions that tests/mrc_reference.py decodes
by, not confirmed against a file written by IMOD or SerialEM.  A sample outside its range is written as its low bits
masked to the field and counted."""

import numpy as np

# (numpy dtype of the movie, mode) -> (lowest, highest) accepted value; the first mode of a dtype is its default
TABLE = {("u1", 0): (0, 255), ("u1", 101): (0, 15),
         ("i2", 1): (-32768, 32767), ("i2", 6): (0, 32767), ("i2", 0): (-128, 127), ("i2", 101): (0, 15)}
KINDS = tuple(TABLE)


def row_bytes(mode, w):
    return (w + 1) // 2 if mode == 101 else w * (1 if mode == 0 else 2)


def encode(movie, mode, flip_rows=False):
    """(t, h, w) uint8 / int16 -> the payload's bytes"""
    movie = np.asarray(movie)
    assert movie.ndim == 3 and (movie.dtype.str[1:], mode) in TABLE
    rows = movie[:, ::-1, :] if flip_rows else movie
    wide = rows.astype(np.int64)
    if mode == 101:
        t, h, w = wide.shape
        padded = np.zeros((t, h, 2 * ((w + 1) // 2)), dtype=np.int64)
        padded[:, :, :w] = wide & 15
        return (padded[:, :, 0::2] | (padded[:, :, 1::2] << 4)).astype(np.uint8).tobytes()
    if mode == 0:
        return (wide & 255).astype(np.uint8).tobytes()
    return (wide & 65535).astype("<u2").tobytes()


def statistics(movie, mode):
    """(t, h, w) -> the (t, 5) int64 table: per frame the minimum, the maximum, the sum, the sum of squares of the
    samples as the movie holds them, and the count of samples outside the mode's range"""
    movie = np.asarray(movie)
    lo, hi = TABLE[(movie.dtype.str[1:], mode)]
    wide = movie.astype(np.int64).reshape(movie.shape[0], -1)
    return np.stack([wide.min(1), wide.max(1), wide.sum(1), (wide * wide).sum(1),
                     ((wide < lo) | (wide > hi)).sum(1)], axis=1).astype(np.int64)


def header_statistics(movie):
    """(dmin, dmax, dmean, rms) of the whole movie in float64 numpy, rms the root of the mean squared deviation"""
    wide = np.asarray(movie).astype(np.float64)
    mean = float(wide.mean())
    return float(wide.min()), float(wide.max()), mean, float(np.sqrt(((wide - mean) ** 2).mean()))


def pixels(dtype, mode, shape, seed=0, spoil=0):
    """A random movie inside the mode's range, the extremes of the range included; `spoil` samples just outside it"""
    lo, hi = TABLE[(dtype, mode)]
    rng = np.random.default_rng([seed, mode, int(dtype[1]), *shape])
    px = rng.integers(lo, hi + 1, shape).astype(dtype)
    flat = px.reshape(-1)
    flat[rng.integers(0, flat.size)] = hi
    flat[rng.integers(0, flat.size)] = lo
    outside = [v for v in (hi + 1, lo - 1, hi + 17, -32768, 32767, 255) if not lo <= v <= hi
               and np.iinfo(dtype).min <= v <= np.iinfo(dtype).max]
    for k in range(spoil if outside else 0):
        flat[rng.integers(0, flat.size)] = outside[k % len(outside)]
    return px
