"""The detector-defect fill rule (DefectFill, fill_defects_raw, fill_defects_gain) restated with numpy and Python
integers only.  Nothing here imports the package.

Defects are listed in row-major order; j is a defect's place in the list, p_j = y * w + x.  The ring at Chebyshev
distance r around (y, x) is the pixels with max(|dy|, |dx|) == r inside the frame.  Defect j's donors are the good
pixels of the first ring r = 1 .. reach that holds any, in row-major order.  Frame f takes

    x = seed ^ (f * 0x9E3779B1) ^ (j * 0x85EBCA77)                                   (uint32, wrapping)
    x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16
    out[f, p_j] = movie[f, donors[j][(x * count_j) >> 32]]

and the gain of a defect is float32(sum of float64(donor gains) in table order / count_j)."""

import numpy as np

M32 = 0xFFFFFFFF


def ring(y, x, r, h, w):
    """The pixels (yy, xx) at Chebyshev distance exactly r from (y, x) inside an (h, w) frame, in row-major order."""
    out = []
    for yy in range(y - r, y + r + 1):
        for xx in range(x - r, x + r + 1):
            if max(abs(yy - y), abs(xx - x)) == r and 0 <= yy < h and 0 <= xx < w:
                out.append((yy, xx))
    return out


def donor_table(defect_map, reach):
    """-> (pixels (n,), donors (n, 8 * reach) with -1 in unused entries, counts (n,)), all int32.  counts[j] == 0
    where no ring up to `reach` holds a good pixel."""
    dmap = np.asarray(defect_map, dtype=bool)
    h, w = dmap.shape
    pixels = [y * w + x for y in range(h) for x in range(w) if dmap[y, x]]
    donors = np.full((len(pixels), 8 * reach), -1, dtype=np.int32)
    counts = np.zeros(len(pixels), dtype=np.int32)
    for j, p in enumerate(pixels):
        y, x = divmod(p, w)
        for r in range(1, reach + 1):
            good = [yy * w + xx for yy, xx in ring(y, x, r, h, w) if not dmap[yy, xx]]
            if good:
                donors[j, :len(good)] = good
                counts[j] = len(good)
                break
    return np.asarray(pixels, dtype=np.int32), donors, counts


def pick(seed, f, j, count):
    """The donor slot of frame f and defect j, in Python integers."""
    x = (seed ^ (f * 0x9E3779B1) ^ (j * 0x85EBCA77)) & M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return (x * count) >> 32


def picks(seed, f, j, count):
    """pick() over numpy arrays of f and / or j (uint64 arithmetic masked to 32 bits) -> int64 array."""
    f, j = np.asarray(f, dtype=np.uint64), np.asarray(j, dtype=np.uint64)
    m = np.uint64(M32)
    x = (np.uint64(seed) ^ ((f * np.uint64(0x9E3779B1)) & m) ^ ((j * np.uint64(0x85EBCA77)) & m)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m
    x ^= x >> np.uint64(16)
    return ((x * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


def first_without_donor(defect_map, reach):
    """(y, x) of the first defect (row-major) without a good pixel within `reach`, or None."""
    pixels, _, counts = donor_table(defect_map, reach)
    w = np.asarray(defect_map).shape[1]
    for p, c in zip(pixels, counts):
        if c == 0:
            return divmod(int(p), w)
    return None


def fill(movie, defect_map, reach, seed, table=None):
    """The filled copy of a (t, h, w) or (h, w) numpy movie of any dtype: elements are copied, never converted."""
    movie = np.ascontiguousarray(movie)
    out = movie.copy()
    pixels, donors, counts = donor_table(defect_map, reach) if table is None else table
    assert counts.min(initial=1) > 0, "a defect has no donor"
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[movie.dtype.itemsize]  # NaN payloads travel as integers
    hw = movie.shape[-2] * movie.shape[-1]
    src, dst = movie.view(bits).reshape(-1, hw), out.view(bits).reshape(-1, hw)
    for f in range(src.shape[0]):
        for j, p in enumerate(pixels):
            dst[f, p] = src[f, donors[j, pick(seed, f, j, int(counts[j]))]]
    return out


def gain_fill(gain, defect_map, reach, table=None):
    gain = np.asarray(gain, dtype=np.float32)
    out = gain.copy()
    pixels, donors, counts = donor_table(defect_map, reach) if table is None else table
    assert counts.min(initial=1) > 0, "a defect has no donor"
    flat_in, flat_out = gain.reshape(-1), out.reshape(-1)
    for j, p in enumerate(pixels):
        s = 0.0  # a Python float is a float64; one add per donor, in table order
        for k in range(int(counts[j])):
            s += float(flat_in[donors[j, k]])
        flat_out[p] = np.float32(s / int(counts[j]))
    return out
